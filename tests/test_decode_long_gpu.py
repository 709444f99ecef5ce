"""qs_single_query_attention_long (csrc/attention_long.hip) against the float64 attention over the de-quantised pool, at LC.TOL:
small shapes where the device-side ranges, the address window and the writer can go wrong, contexts past the 192-entry tables of the
other matrix-core kernels (the aliased construction of tests/_long_cases.py, its host conditions asserted over the ranges the launch
uses), a RoPE profile key, and a captured call replayed while the lengths grow."""
import functools

import numpy as np
import pytest
import torch

import _attn_cases as AC
import _long_cases as LC
import _rope_scaling_cases as RC
from _append_cases import host_pool, rotate_rows, scattered_tables
from _helpers import DevPools, dev
from oracle import kvattn

pytestmark = pytest.mark.gpu
TOL = LC.TOL
KV = [pytest.param(True, id="kv4"), pytest.param(False, id="kv8")]
PASTS, MB = [0, 63, 64, 200], 8      # only the new token; the last slot of a page; the first of a fresh page; a partly filled fourth page


def _np(t):
    return t.detach().cpu().numpy()


def _call(new, kvp, lengths, H, Hkv, int4, base, timestep, splits):
    from qserve_amd.long_decode import single_query_attention_long
    q, k, v = [x.reshape(new.size(0), -1, 128) for x in new.split([H * 128, Hkv * 128, Hkv * 128], dim=-1)]
    return single_query_attention_long(q, k, v, kvp, lengths, Hkv * (64 if int4 else 128), timestep, base, int4, num_splits=splits)


@functools.lru_cache(maxsize=None)
def _small(H, Hkv, int4, profile):
    """Four sequences of PASTS cached tokens under tables of MB entries: host pool, new rows, and - once - the oracle's output and pools."""
    from qserve_amd import rope
    prof = rope.profile(RC.BASE, RC.LLAMA3) if profile else (rope.base_denominators(RC.BASE), np.float32(1.0))
    key = rope.register(prof[0], prof[1], 2048) if profile else RC.BASE
    r = np.random.default_rng(11 + 8 * H + Hkv + int(int4))
    tables, nblocks = scattered_tables(r, len(PASTS), MB)
    host0 = kvattn.PagePool(nblocks, Hkv, 128, int4, fill=0xFF)
    RC.history(host0, r, tables, PASTS, H, Hkv, prof)
    new = r.standard_normal((len(PASTS), (H + 2 * Hkv) * 128)).astype(np.float16)
    lengths = np.asarray(PASTS, np.int32) + 1
    ref, want_k, want_v = RC.expect_decode(host0, new, lengths, tables, H, Hkv, prof)
    return dict(key=key, tables=tables, nblocks=nblocks, host0=host0, new=new, lengths=lengths, ref=ref, want_k=want_k, want_v=want_v)


def _run_small(c, H, Hkv, int4, splits):
    pools = DevPools(c["nblocks"], Hkv, int4, "cuda:0")
    pools.k.copy_(dev(c["host0"].k)), pools.v.copy_(dev(c["host0"].v))
    out = _call(dev(c["new"]), pools.pointers(c["tables"]), dev(c["lengths"]), H, Hkv, int4, c["key"], MB * 64, splits)
    torch.cuda.synchronize()
    return _np(out), _np(pools.k), _np(pools.v)


def _check_small(c, H, Hkv, int4, splits, what):
    out, k, v = _run_small(c, H, Hkv, int4, splits)
    err = float(np.abs(out.astype(np.float32) - c["ref"]).max())
    print(f"DECODELONG {what} H={H} Hkv={Hkv} int4={int4} splits={splits}: max abs err {err:.3e}")
    assert np.isfinite(out.astype(np.float32)).all() and err <= TOL, f"max abs err {err:.2e}"
    assert np.array_equal(k, c["want_k"]), "K pages: the new token's slot against kv_quantize of the rotated row, or a byte elsewhere"
    assert np.array_equal(v, c["want_v"]), "V pages: the new token's slot, or a byte elsewhere"
    again = _run_small(c, H, Hkv, int4, splits)
    assert all(np.array_equal(a, b) for a, b in zip((out, k, v), again)), "a second run differs"


@pytest.mark.parametrize("splits", [1, 3, 64])
@pytest.mark.parametrize("H,Hkv", [(8, 8), (8, 2), (8, 1), (5, 1)])
@pytest.mark.parametrize("int4", KV)
def test_small_shapes_ranges_window_and_writer(gpu, int4, H, Hkv, splits):
    """splits = 3 and 64 ask for more ranges than a sequence has pages: empty records; 200 tokens are two ranges of two pages."""
    _check_small(_small(H, Hkv, int4, False), H, Hkv, int4, splits, "small")


def test_profile_key_as_the_base(gpu):
    _check_small(_small(8, 2, True, True), 8, 2, True, 3, "llama3 profile")


# ---- past the old limit: the aliased long context of tests/_long_cases.py ---------------------------------------------------------------
def _pools(case):
    """0xFF everywhere, the case's 8 + B history pages written by the existing prefill writer."""
    from qserve_backend import fused_attention as fa
    pools = DevPools(case.nblocks, case.Hkv, case.int4, "cuda:0")
    n = case.hist_len
    fa.apply_bias_rope_update_kv_cache(dev(case.hist), dev(np.asarray([n], np.int32)),
                                       fa.compute_padding_offsets(dev(np.asarray([0, n], np.int32)), n, n), pools.pointers(case.hist_tables),
                                       case.H, case.Hkv, n, 64, case.spt, 128, LC.BASE, 8192, True, case.int4, True)
    torch.cuda.synchronize()
    return pools


@pytest.mark.parametrize("int4", KV)
@pytest.mark.parametrize("L", [12289, 33000, LC.LONGEST + 1])
def test_past_the_old_limit(gpu, L, int4):
    """The planner's count and one range (longer than any address window), over one reference; the written slot bit for bit."""
    from qserve_amd.long_decode import page_ranges
    from qserve_amd.plan import attention_long_plan
    case = LC.decode_case(int4, L)
    H, Hkv, B = case.H, case.Hkv, case.B
    plan = attention_long_plan(B, H, Hkv, case.mb, int4)
    assert plan["splits"] > 1, plan
    pools = _pools(case)
    hp = host_pool(_np(pools.k), _np(pools.v), Hkv, int4)
    rot = rotate_rows(case.new, case.cu_q, case.past, H, Hkv, LC.BASE)
    refs, ref = LC.references(case, rot, hp)
    sets = [page_ranges(int(p) + 1, plan["splits"], plan["min_pages"]) + page_ranges(int(p) + 1, 1, plan["min_pages"]) for p in case.past]
    LC.conditions(case, refs, sets, f"decode long L={L} int4={int4}", AC.SENS)
    kb, ks, kz = kvattn.kv_quantize(rot[:, H * 128:(H + Hkv) * 128].reshape(B, Hkv, 128), int4)
    vb, vs, vz = kvattn.kv_quantize(case.new[:, (H + Hkv) * 128:].reshape(B, Hkv, 128), int4)
    for b in range(B):
        pos = int(case.past[b])
        for h in range(Hkv):
            hp.write_token("k", int(case.tables[b, 0, pos // 64]), pos % 64, h, kb[b, h], ks[b, h], kz[b, h])
            hp.write_token("v", int(case.tables[b, 1, pos // 64]), pos % 64, h, vb[b, h], vs[b, h], vz[b, h])
    before = pools.k.clone(), pools.v.clone()
    for splits in (0, 1):
        pools.k.copy_(before[0]), pools.v.copy_(before[1])
        out = _call(dev(case.new), pools.pointers(case.tables), dev(case.past + 1), H, Hkv, int4, LC.BASE, L, splits)
        torch.cuda.synchronize()
        got = _np(out).astype(np.float32)
        err = float(np.abs(got - ref.reshape(got.shape)).max())
        print(f"DECODELONG L={L} int4={int4} B={B} splits={splits or plan['splits']}: max abs err {err:.3e}")
        assert np.array_equal(_np(pools.k), hp.k) and np.array_equal(_np(pools.v), hp.v), "pages: the new token's slot, or a byte elsewhere"
        assert np.isfinite(got).all() and err <= TOL, f"splits={splits}: max abs err {err:.2e}"


@pytest.mark.parametrize("int4", KV)
def test_captured_call_follows_the_lengths(gpu, int4):
    """B = 2 under a 520-entry table at pasts (127, 33 000): three replays, the lengths advanced on the device between them - the first
    sequence crosses into a fresh page -, each equal to an eager call at the same lengths, outputs and pools, bit for bit."""
    case = LC.Case(8, 2, int4, [127, 33000], [4, 4], 520, 77 + int(int4))
    H, Hkv = case.H, case.Hkv
    graph_pools, eager_pools = _pools(case), _pools(case)
    kvp_g, kvp_e = graph_pools.pointers(case.tables), eager_pools.pointers(case.tables)
    rows = dev(case.new).view(2, 4, -1)
    new, lengths = rows[:, 0].clone(), dev(case.past + 1)
    _call(new, kvp_g, lengths, H, Hkv, int4, LC.BASE, 520 * 64, 0)            # outside the capture: the split-KV workspace's first use
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = _call(new, kvp_g, lengths, H, Hkv, int4, LC.BASE, 520 * 64, 0)
    for i in range(3):
        new.copy_(rows[:, i])
        g.replay()
        eager = _call(new, kvp_e, lengths, H, Hkv, int4, LC.BASE, 520 * 64, 0)
        torch.cuda.synchronize()
        assert torch.isfinite(out.float()).all() and torch.equal(out, eager), f"replay {i}: output differs from the eager call"
        assert torch.equal(graph_pools.k, eager_pools.k) and torch.equal(graph_pools.v, eager_pools.v), f"replay {i}: pages differ"
        lengths.add_(1)
