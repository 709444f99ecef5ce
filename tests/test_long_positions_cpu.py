"""Host side of the long-context tests (no GPU): the oracle's RoPE coefficients at the positions the GPU tests reach, pinned against an
independent element-by-element evaluation; the aliased long-context construction of tests/_long_cases.py with its three conditions on
the quantised float64 reference; and the cost of one reference at the longest length the GPU tests use."""
import math
import time

import numpy as np
import pytest

import _attn_cases as AC
import _long_cases as LC
from _append_cases import expected, rotate_rows
from oracle import kvattn

POSITIONS = [0, 1, 2047, 2048, 8191, 8192, 12287, 12288, 32767, 32768, 65535, 65536, 131071]
BASES = [1e4, 5e5, 1e6]

try:
    import mpmath
except ImportError:      # Python's math on the same float32 inputs, element by element
    mpmath = None


def _independent(pos, i, base):
    """(cos, sin) of rotary pair i at `pos`: every step on float(np.float32(...)) inputs, evaluated to double precision and rounded once
    to float32 - with mpmath at 60 digits and one rounding to double, otherwise with Python's math (the C library's double functions)."""
    f32 = lambda x: float(np.float32(x))      # noqa: E731
    expo = f32(f32(2 * i) / f32(128))
    if mpmath is not None:
        with mpmath.workprec(200):
            denom = f32(float(mpmath.power(mpmath.mpf(f32(base)), mpmath.mpf(expo))))
            ang = f32(f32(pos) / denom)
            return f32(float(mpmath.cos(mpmath.mpf(ang)))), f32(float(mpmath.sin(mpmath.mpf(ang))))
    denom = f32(math.pow(f32(base), expo))
    ang = f32(f32(pos) / denom)
    return f32(math.cos(ang)), f32(math.sin(ang))


@pytest.mark.parametrize("base", BASES)
def test_rope_coef_is_pinned_at_long_positions(base):
    worst = 0
    for pos in POSITIONS:
        c, s = kvattn.rope_coef(pos, 128, base)
        assert c.dtype == np.float32 and s.dtype == np.float32 and c.shape == (64,)
        want = np.array([_independent(pos, i, base) for i in range(64)], np.float32)
        assert np.array_equal(c.view(np.uint32), want[:, 0].view(np.uint32)), (base, pos, "cos")
        assert np.array_equal(s.view(np.uint32), want[:, 1].view(np.uint32)), (base, pos, "sin")
        worst = max(worst, pos)
    print(f"base {base:g}: 64 pairs x {len(POSITIONS)} positions up to {worst} bit-equal to the "
          f"{'mpmath' if mpmath is not None else 'math'} evaluation")


def test_the_table_aliases_eight_pages_and_keeps_own_pages_for_new_tokens():
    case = LC.Case(8, 2, True, [LC.LONG, 60 + 64 * 300], [8, 8], 520, 1, shared_pages=256)      # (a table layout only: not a GPU case)
    k = case.tables[:, 0]
    full = LC.LONG // 64
    assert full == 515 and LC.LONG % 64 == 40
    assert np.array_equal(k[0, :full], (8 * np.arange(full)) // full) and sorted(set(k[0, :full].tolist())) == list(range(8))
    assert k[0, full] == 8 and (k[0, full + 1:] == case.dummy).all()                 # 40 + 8 <= 64: the tail page takes the new tokens
    assert np.array_equal(k[1, :256], k[0, :256]) and np.array_equal(k[1, 256:300], (8 * np.arange(256, 300)) // 300)
    assert k[1, 300] == 9 and k[1, 301] == 10 and (k[1, 302:] == case.dummy).all()   # 60 + 8 > 64: one fresh page behind the tail
    assert case.spare not in k and case.vperm[case.spare] not in case.tables[:, 1] and case.nblocks == 13
    assert np.array_equal(case.tables[:, 1], case.vperm[k])
    # the offsets: per dimension four of the 8 history pages carry + C, four - C
    assert ((case.sign[:8] > 0).sum(axis=0) == 4).all() and (np.abs(case.sign) == 1).all()
    v = case.hist[:, (8 + 2) * 128:].astype(np.float32).reshape(10, 64, 2, 128)
    assert np.abs(v.mean(axis=(1, 2)) - LC.C * case.sign).max() < 0.5
    # the pool: the prefill oracle wrote the 8 + 2 pages and nothing else
    pool = case.host_pages(1e6)
    rest = [p for p in range(case.nblocks) if p >= 10]
    assert (pool.k[rest] == 0xFF).all() and (pool.v[case.vperm[rest]] == 0xFF).all()
    assert not (pool.k[:10] == 0xFF).all(axis=1).any()


def test_split_ranges_restate_the_device_rule():
    assert LC.split_ranges(LC.LONG, 8) == [(65 * 64 * s, min(65 * 64 * (s + 1), LC.LONG)) for s in range(8)]
    r64 = LC.split_ranges(LC.LONG, 64)                       # 516 pages, 9 per split: 58 ranges, the last of 3 pages (2 full + 40 tokens)
    assert len(r64) == 58 and r64[0] == (0, 576) and r64[-1] == (57 * 576, LC.LONG)
    assert LC.split_ranges(100, 64) == [(0, 64), (64, 100)]
    assert LC.split_ranges(64 * 300 + 60, 4, page0=256) == [(64 * 256 + 64 * 12 * s, min(64 * 256 + 64 * 12 * (s + 1), 64 * 300 + 60)) for s in range(4)]
    assert [e for _, e in LC.eighths(LC.LONG)][-1] == LC.LONG


def _conditions(case, sets, what):
    pool = case.host_pages(LC.BASE)
    rot = rotate_rows(case.new, case.cu_q, case.past, case.H, case.Hkv, LC.BASE)
    refs, ref = LC.references(case, rot, pool)
    LC.conditions(case, refs, sets, what, AC.SENS)
    return rot, pool, ref


@pytest.mark.parametrize("int4", [True, False], ids=["kv4", "kv8"])
@pytest.mark.parametrize("H,Hkv", [(8, 2), (8, 1)])
def test_conditions_hold_for_the_append_cases_at_33000(H, Hkv, int4):
    """The GPU tests' append case (two sequences, 8 new rows each): an eighth, and every range of 8 or 64 splits, of the planner's count and
    of the shared-prefix launch, moves every row of the quantised reference; the removable-range reference is the flash oracle's."""
    from qserve_amd.plan import append_attention_split_plan
    case = LC.append_case(H, Hkv, int4, False)
    plan = append_attention_split_plan(case.B, 8, int(case.past.max()), H, Hkv, int4)
    assert 1 < plan["splits"] <= 64
    rot, pool, ref = _conditions(case, LC.append_split_sets(case, (plan["splits"],)), f"append H={H} Hkv={Hkv} int4={int4}")
    want = expected(rot, case.cu_q, case.past, case.tables, pool, H, Hkv)
    assert np.abs(ref - want).max() <= 1e-6, "the removable-range reference is not the flash oracle's composition"


@pytest.mark.parametrize("int4", [True, False], ids=["kv4", "kv8"])
@pytest.mark.parametrize("L", [8192, 12289, 32769])
def test_conditions_hold_for_the_decode_cases(L, int4):
    """n = 1: the matrix-core families' 8 KV splits at 8 192, the VALU family behind 192 pages."""
    from qserve_amd.plan import attention_plan
    case = LC.decode_case(int4, L)
    plan = attention_plan(case.B, 8, 2, case.mb, L, int4)
    assert (plan["family"] == "valu") == (case.mb > 192)
    sets = [LC.decode_split_ranges(int(p), plan["kv_splits"], int4) if plan["kv_splits"] > 1 else [] for p in case.past]
    _conditions(case, sets, f"decode L={L} int4={int4}")


def test_conditions_and_cost_at_the_longest_length():
    """The longest attention length of the GPU tests: one reference (composition from the pages + float64 attention) is timed."""
    t0 = time.process_time()
    w0 = time.perf_counter()
    case = LC.Case(8, 2, True, [LC.LONGEST], [8], 2048, 5)
    pool = case.host_pages(LC.BASE)
    refs, ref = LC.references(case, rotate_rows(case.new, case.cu_q, case.past, 8, 2, LC.BASE), pool)
    cpu, wall = time.process_time() - t0, time.perf_counter() - w0
    print(f"one reference at {LC.LONGEST} tokens, 8 new rows, 8 / 2 heads: {wall:.2f} s wall, {cpu:.2f} s CPU")
    assert wall < 10.0, f"the long reference took {wall:.1f} s: shorten _long_cases.LONGEST"
    LC.conditions(case, refs, [LC.split_ranges(LC.LONGEST, 8) + LC.split_ranges(LC.LONGEST, 64)], "longest", AC.SENS)
