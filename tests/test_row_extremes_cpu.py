"""The row-kernel cases of tests/_row_extreme_cases.py are what they claim (no GPU): the width tables and the restated selection rules
follow from the constants qserve_amd/csrc/fused_small.hip and row_ops.h state TODAY (a changed launcher rule fails here), every
instantiation a launcher can select is reached, the tie rows are ties, the planted positions reach the partial last chunk, the
cancelling planes cancel only in integers, and the oracle's answers on NaN / inf / subnormal / flat rows equal hand-written
expectations taken from the reference source."""
import os
import re

import numpy as np
import pytest

import _row_extreme_cases as rc
from oracle import fused

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "qserve_amd", "csrc")


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


@pytest.fixture(scope="module")
def src():
    hip = _read("fused_small.hip")

    def entry(name):
        m = re.search(r'extern "C" int %s\(.*?\n}\n' % name, hip, re.S)
        assert m, name
        return m.group(0)
    return dict(hip=hip, h=_read("row_ops.h"), entry=entry)


def _int(pattern, text):
    m = re.search(pattern, text)
    assert m, pattern
    return int(m.group(1))


def _consts(src):
    tpb = _int(r"constexpr int TPB = (\d+);", src["hip"])
    return dict(TPB=tpb, WIDE_ROW=_int(r"constexpr int WIDE_ROW = (\d+);", src["h"]), ROW=tpb * 8)


def _parsed_quant_rule(body, macro, var, c):
    """(NC, NT) as the launcher text selects it: `if (var > WIDE_ROW) { if (var <= a) M(..); else if (var <= b) M(..); else M(..); }
    else { nc = ceil(var / (TPB * 8)); if (nc == 1) M(1, TPB); else M(2, TPB); }`."""
    limit = _int(r"%s <= (\d+), \"" % var, body)
    wide = re.search(r"if \(%s > WIDE_ROW\) \{(.*?)\} else \{(.*?)\n    \}" % var, body, re.S)
    assert wide, "the geometry rule no longer has the shape this test parses"
    steps = [(int(a), int(nc), int(nt)) for a, nc, nt in re.findall(r"if \(%s <= (\d+)\) %s\((\d+), (\d+)\);" % (var, macro), wide.group(1))]
    last = re.search(r"else %s\((\d+), (\d+)\);" % macro, wide.group(1))
    assert len(steps) == 2 and last
    assert re.search(r"const int nc = \(%s \+ TPB \* 8 - 1\) / \(TPB \* 8\);" % var, wide.group(2))
    narrow = re.search(r"if \(nc == 1\) %s\((\d+), TPB\);\s*else %s\((\d+), TPB\);" % (macro, macro), wide.group(2))
    assert narrow

    def rule(h):
        if h > c["WIDE_ROW"]:
            for a, nc, nt in steps:
                if h <= a:
                    return (nc, nt)
            return (int(last.group(1)), int(last.group(2)))
        return (int(narrow.group(1)) if -(-h // c["ROW"]) == 1 else int(narrow.group(2)), c["TPB"])
    return limit, rule, [a for a, _, _ in steps]


def test_constants_are_the_sources(src):
    c = _consts(src)
    assert (c["TPB"], c["WIDE_ROW"]) == (rc.TPB, rc.WIDE_ROW) and rc.ROW == rc.TPB * rc.CHUNK
    assert "constexpr int WIDE_ROW = qs_row::WIDE_ROW;" in src["hip"]
    assert _int(r"\(hidden \+ (\d+)\) / 512", src["h"]) == rc.BLOCK - 1                      # quant_row's nblk
    assert _int(r"\(d \+ (\d+)\) / 512", src["hip"]) == rc.BLOCK - 1                         # silu_mul_quant_kernel's nblk
    assert _int(r"if \(chunks > (\d+)\) chunks = \1;", src["entry"]("qs_silu_and_mul")) == rc.SILU_MAX_CHUNKS
    assert "(d + TPB * 8 - 1) / (TPB * 8)" in src["entry"]("qs_silu_and_mul")
    assert _int(r"if \(blocks > (\d+)\) blocks = \1;", src["entry"]("qs_residual_add")) == rc.RESADD_MAX_BLOCKS
    assert "(n8 + TPB - 1) / TPB" in src["entry"]("qs_residual_add")
    assert "i += TPB * 8" in src["hip"]                                                      # rms_norm_kernel's trip


@pytest.mark.parametrize("name,macro,var", [("qs_invoke_quant", "QS_Q", "hidden"), ("qs_silu_and_mul_quant", "QS_S", "d")])
def test_quant_rule_and_widths_follow_the_launcher(src, name, macro, var):
    c = _consts(src)
    limit, rule, steps = _parsed_quant_rule(src["entry"](name), macro, var, c)
    assert limit == rc.QUANT_MAX
    for h in range(8, limit + 1, 8):
        assert rule(h) == rc.quant_inst(h), h
    # the table: 8, every boundary of the parsed rule and one chunk past it, the limit
    bounds = [rc.BLOCK, c["ROW"], c["WIDE_ROW"]] + steps
    want = sorted({8, limit} | {b + o for b in bounds for o in (0, 8)})
    assert list(rc.QUANT_WIDTHS) == want == [8, 512, 520, 2048, 2056, 4096, 4104, 8192, 8200, 16384, 16392, 32768]
    assert {rule(h) for h in rc.QUANT_WIDTHS} == rc.ALL_QUANT_INST
    assert {(int(a), int(b)) for a, b in re.findall(r"%s\((\d+), (\d+|TPB)\)" % macro, src["entry"](name).replace("TPB)", "%d)" % c["TPB"]))} \
        == rc.ALL_QUANT_INST, "an instantiation the rule above never selects"
    # one width per boundary changes the instantiation, its neighbour one chunk on keeps or changes it as the rule says
    for b in (c["ROW"], c["WIDE_ROW"], *steps):
        assert rule(b) != rule(b + 8)


def _parsed_norm_switch(body):
    sw = re.search(r"switch \(nc\) \{(.*?)\n    \}", body, re.S).group(1)
    table = {}
    for labels, nc in re.findall(r"((?:case \d+: )+)QS_N\((\d+)\); break;", sw):
        for k in re.findall(r"case (\d+):", labels):
            table[int(k)] = int(nc)
    default = _int(r"default: QS_N\((\d+)\); break;", sw)
    return table, default


def test_norm_rules_and_widths_follow_the_launchers(src):
    c = _consts(src)
    for name in ("qs_rms_norm_general", "qs_add_residual_rms_norm_general"):
        body = src["entry"](name)
        assert re.search(r"hidden <= 8 \* TPB \* 8,", body) and rc.NORM_MAX == 8 * c["TPB"] * 8
        assert "const int nc = (hidden + TPB * 8 - 1) / (TPB * 8);" in body
        assert "const bool refsum = g_row_refsum && input_sum;" in body
        table, default = _parsed_norm_switch(body)
        for h in range(8, rc.NORM_MAX + 1, 8):
            nc = table.get(-(-h // c["ROW"]), default)
            assert rc.norm_inst(h, False)[0] == nc == rc.add_norm_inst(h, True)[0], h
    add = src["entry"]("qs_add_residual_rms_norm_general")
    # refsum first (never FULL), then FULL exactly at NC * TPB * 8
    assert re.search(r"if \(refsum\)\s*\\\s*hipLaunchKernelGGL\(\(add_residual_norm_quant_kernel<NC, false, true>\)", add)
    assert re.search(r"else if \(hidden == NC \* TPB \* 8\)\s*\\\s*hipLaunchKernelGGL\(\(add_residual_norm_quant_kernel<NC, true>\)", add)
    assert re.search(r"else\s*\\\s*hipLaunchKernelGGL\(\(add_residual_norm_quant_kernel<NC, false>\)", add)
    bounds = sorted({k * c["ROW"] for k in table})                    # every ceil(H / 2048) the switch names: 2048 .. 8192
    want = sorted({8, rc.NORM_MAX} | {b + o for b in bounds for o in (0, 8)})
    assert list(rc.NORM_WIDTHS) == want == [8, 2048, 2056, 4096, 4104, 6144, 6152, 8192, 8200, 16384]
    assert {rc.norm_inst(h, r) for h in rc.NORM_WIDTHS for r in (False, True)} == rc.ALL_NORM_INST
    assert {rc.add_norm_inst(h, r) for h in rc.NORM_WIDTHS for r in (False, True)} == rc.ALL_ADD_NORM_INST
    assert rc.add_norm_inst(6144, False) == (4, False, False) and rc.add_norm_inst(8192, False) == (4, True, False)
    assert len(rc.ALL_NORM_INST) == 8 and len(rc.ALL_ADD_NORM_INST) == 12


def test_planes_rule_and_cases_follow_the_launcher(src):
    c = _consts(src)
    body = src["entry"]("qs_add_residual_rms_norm_general_planes")
    assert re.search(r"hidden <= 2 \* TPB \* 8,", body) and rc.PLANES_MAX == 2 * c["TPB"] * 8
    assert "k_slices == 1 || k_slices == 2 || k_slices == 4" in body and rc.PLANES_KS == (1, 2, 4)
    assert "if (nc == 1) QS_PK(1, 0);" in body and "else QS_PK(2, 0);" in body and "if (nc == 1) QS_PK(1, 1);" in body
    assert re.search(r"if \(refsum\) \{\s*\\\s*constexpr bool FULLV = false, REFV = true;", body)
    assert re.search(r"\} else if \(hidden == NC \* TPB \* 8\) \{", body)
    assert list(rc.PLANES_WIDTHS) == [8, 1024, 2040, 2048, 2056, 3072, 4088, 4096]
    got = {rc.planes_inst(h, ks, m == "per_group", ref) for h, ks, m, ref, _ in rc.planes_cases()}
    assert got == rc.ALL_PLANES_INST and len(got) == 36
    assert {(m, ref) for _, _, m, ref, _ in rc.planes_cases()} == {(m, r) for m in rc.PLANES_MODES for r in (False, True)}


def test_loop_trips():
    assert [rc.silu_trips(d) for d in rc.SILU_WIDTHS] == [1, 1, 1, 2, 2] and list(rc.SILU_WIDTHS) == [8, 2048, 32768, 32776, 65536]
    assert [rc.resadd_trips(n) for n in rc.RESADD_SIZES] == [1, 1, 2, 4]
    assert list(rc.RESADD_SIZES) == [8, 4194304, 4194312, 3 * 4194304 + 24]
    assert list(rc.RMS_WIDTHS) == [8, 2048, 2056, 4104, 16392]


# ---- the rows ---------------------------------------------------------------------------------------------------------------------
def test_batches_have_three_to_eight_rows_and_are_fp16():
    for h in (8, 520, 2056, 6152):
        for b in rc.add_norm_batches(h) + rc.silu_quant_batches(h):
            rows = b.rows if b.pair is None else b.pair[0]
            assert rows.dtype == np.float16 and 3 <= rows.shape[0] <= 8 and rows.shape[1] == h and len(b.notes) == rows.shape[0]


@pytest.mark.parametrize("h", sorted(set(rc.QUANT_WIDTHS) | set(rc.NORM_WIDTHS)))
def test_planted_positions_cover_the_partial_last_chunk(h):
    for nt in {rc.TPB, rc.quant_inst(h)[1] if h <= rc.QUANT_MAX else rc.TPB}:
        for fam in (rc.planted, rc.one_hot):
            notes = [n for b in fam(h, nt) for n in b.notes if "pos" in n]
            pos = {n["pos"] for n in notes}
            assert {0, 7, h - 8, h - 1} <= pos and {c * nt * 8 for c in range(-(-h // (nt * 8)))} <= pos
            if h > rc.BLOCK:
                assert rc.BLOCK - 1 in pos
            assert any(n["last_chunk"] for n in notes)
            if h % (nt * 8):
                assert any(n["partial_set"] and n["last_chunk"] for n in notes), "no maximum in the partial last chunk set"
            for b in fam(h, nt):
                for row, n in zip(b.rows, b.notes):
                    if "pos" in n:
                        a = np.abs(row.astype(np.float32))
                        assert a.argmax() == n["pos"] and (a > a[n["pos"]] / 2).sum() == 1
    for fam in (rc.planted, rc.one_hot):                                          # both signs at every position
        signs = {(n["pos"], np.sign(float(b.rows[i, n["pos"]]))) for b in fam(h, rc.TPB) for i, n in enumerate(b.notes) if "pos" in n}
        assert signs == {(p, s) for p in rc.planted_positions(h, rc.TPB) for s in (1.0, -1.0)}
    for b in rc.one_hot(h, rc.TPB):
        for row, n in zip(b.rows, b.notes):
            if "pos" in n:
                assert (row.view(np.uint16) != 0).sum() == 1                      # everything else is +0.0, bit for bit


@pytest.mark.parametrize("h", [8, 520, 4104, 32768])
def test_tie_rows_are_exact_ties(h):
    (b,) = rc.ties(h)
    q, scale, s, pre = fused.quant_per_token(b.rows, with_sum=True, sum_order="hip")
    assert pre.dtype == np.float32 and np.array_equal(scale, np.full(3, np.float16(1.0)))
    for r in range(3):
        m = b.notes[r]["tie"]
        assert np.array_equal(pre[r, m] - np.floor(pre[r, m]), np.full(m.sum(), np.float32(0.5)))
        assert (q[r, m] % 2 == 0).all(), "ties round to even"
        assert q[r, 0] == 127 and q[r, 1] == -127 and q.min() > -128
    if h >= 256:
        assert set(np.unique(pre[0, b.notes[0]["tie"]])) == set(rc.TIE_VALUES)


def test_cancelling_planes_sum_in_int32_and_not_in_fp32():
    for ks in (2, 4):
        planes, acc = rc.planes_problem(4, 2056, ks, "cancel")
        assert planes.dtype == np.int32 and np.array_equal(planes.astype(np.int64).sum(axis=0), acc)
        assert np.array_equal(planes.sum(axis=0, dtype=np.int32), acc)
        f = np.zeros(acc.shape, np.float32)
        for z in range(ks):
            f = (f + planes[z].astype(np.float32)).astype(np.float32)
        assert (f != acc.astype(np.float32)).mean() > 0.5, "converted plane by plane, the low bits must be lost"
        assert np.abs(acc).max() == rc.ACC_MAX
    for ks in (1, 2, 4):
        planes, acc = rc.planes_problem(4, 1024, ks, "random")
        assert np.array_equal(planes.astype(np.int64).sum(axis=0), acc)


# ---- the oracle -------------------------------------------------------------------------------------------------------------------
def _old_quant_amax(x):
    return np.abs(np.asarray(x, np.float16).astype(np.float32)).max(axis=-1)


def test_running_amax_changes_nothing_for_nan_free_rows():
    """The restated maximum is np.max for NaN-free rows: on the Gaussian cases of tests/test_fused_gpu.py (and the oracle self-tests of
    tests/test_oracle_golden.py) the old and the new formula give the same bits, so no recorded value moves.  No fixture under
    tests/golden/ holds an output of oracle.fused."""
    for T, H in [(1, 64), (5, 4096), (3, 14336), (2, 8192), (7, 256)]:
        x = (np.random.default_rng(T + H).standard_normal((T, H)) * 2).astype(np.float16)
        assert np.array_equal(fused.running_amax(x.astype(np.float32), 0.0), _old_quant_amax(x))
    for T, H in [(1, 64), (4, 4096), (2, 8192), (3, 5120), (5, 512)]:
        r = np.random.default_rng(T * 7 + H)
        x = (r.standard_normal((T, H)) * 1.5 + 0.3).astype(np.float16)
        old = np.maximum(np.abs(x).max(axis=-1), np.float16(1e-6))
        new = fused.running_amax(x, 1e-6)
        assert new.dtype == np.float16 and np.array_equal(new.view(np.uint16), old.view(np.uint16))
    z = np.zeros((2, 64), np.float16)
    assert np.array_equal(fused.running_amax(z, 1e-6), np.full(2, np.float16(1e-6)))
    gold = os.path.join(os.path.dirname(__file__), "golden")
    with open(os.path.join(gold, "make_golden.py")) as f:
        assert "fused" not in f.read()


def test_oracle_runs_every_family():
    for h in (8, 520, 2056):
        for b in rc.quant_batches(h):
            fused.quant_per_token(b.rows, with_sum=True, sum_order="hip")
        for b in rc.add_norm_batches(h):
            with np.errstate(over="ignore"):
                x = b.rows if b.pair is None else (b.pair[0] + b.pair[1])
            g = rc.default_gamma(h) if b.gamma is None else b.gamma
            for so in ("hip", "reference"):
                fused.rms_norm_general(x, g, 1e-5, with_sum=True, sum_order=so, stats_order="hip")
        for b in rc.silu_quant_batches(h):
            g, u = rc.split_for_silu(b.rows) if b.pair is None else b.pair
            fused.quant_per_token(fused.silu_and_mul(np.concatenate([g, u], axis=1)), with_sum=True, sum_order="hip")
        fused.silu_and_mul(rc.silu_regions(h))
        fused.rms_norm(rc.rms_exact_rows(h), rc.default_gamma(h), 1e-5)


def test_oracle_on_nan_and_inf_rows_follows_the_reference():
    """fused_kernels.cu:111-113: `val = val > zero ? val : -val; if (val > amax_val) amax_val = val;` - both comparisons are false for a
    NaN, so the maximum is that of the other elements; :126-129 then quantise those as usual and cvt.rni.sat.s8 of the NaN itself is 0;
    the fp32 sum (:110) is NaN.  An inf element: amax = inf, scale = half(inf / 127) = inf (:121), tmp_scale = 127 / inf = 0 (:126),
    finite * 0 = 0 and inf * 0 = NaN -> 0."""
    h = 520
    x = rc.gaussian(3, h, 20)
    clean = fused.quant_per_token(x, with_sum=True, sum_order="hip")
    xn = x.copy()
    xn[1, h - 1] = np.nan
    q, scale, s, _ = fused.quant_per_token(xn, with_sum=True, sum_order="hip")
    amax = np.abs(x[1, :h - 1].astype(np.float32)).max()
    assert scale[1] == np.float16(amax / np.float32(127)) and np.isfinite(scale).all()
    want = np.rint(x[1, :h - 1].astype(np.float32) * (np.float32(127) / amax))
    assert np.array_equal(q[1, :h - 1], want.astype(np.int8)) and q[1, h - 1] == 0 and np.abs(q[1]).max() == 127
    assert np.isnan(s[1]) and np.array_equal(q[[0, 2]], clean[0][[0, 2]]) and np.array_equal(s[[0, 2]], clean[2][[0, 2]])
    q, scale, s, _ = fused.quant_per_token(np.full((1, 8), np.nan, np.float16), with_sum=True, sum_order="hip")
    assert not q.any() and scale[0] == 0 and np.isnan(s[0])                                  # amax stays 0.0f (:104)
    xi = x.copy()
    xi[1, 0] = -np.inf
    q, scale, s, _ = fused.quant_per_token(xi, with_sum=True, sum_order="hip")
    assert not q[1].any() and np.isposinf(scale[1]) and np.isneginf(s[1])
    xi[1, 5] = np.inf
    assert np.isnan(fused.quant_per_token(xi, with_sum=True, sum_order="hip")[2][1])         # inf + -inf


def test_oracle_norm_on_nan_inf_flat_and_subnormal_rows_follows_the_reference():
    """layernorm_kernels.cu:222,238,243: a NaN (or inf) element makes the mean NaN (inf), :258-265 the variance NaN, so every normalised
    value (:281) is NaN; :285 `amax = cuda_max(cuda_abs(val), amax)` = `(|val| > amax) ? |val| : amax` (utils.cuh:416-420) keeps the
    start value half(1e-6) (:274); :322 scale = half(half(1e-6) / 127) = 0 in fp16; :317-318 NaN * (127 / amax) -> int8 0; :286,323 the
    sum is NaN.  A constant row: mean exact, variance 0, every value 0 - the same scale 0 and int8 row 0, but sum 0."""
    h = 520
    g = rc.default_gamma(h)
    x = rc.ordinary_rows(h)[[0, 1, 0]].copy()
    for bad in (np.nan, np.inf, -np.inf):
        xb = x.copy()
        xb[1, h - 1] = bad
        for so in ("hip", "reference", "fp32"):
            q, scale, s, _ = fused.rms_norm_general(xb, g, 1e-5, with_sum=True, sum_order=so, stats_order="hip")
            assert not q[1].any() and scale[1].view(np.uint16) == 0 and np.isnan(s[1]), (bad, so)
            c = fused.rms_norm_general(x, g, 1e-5, with_sum=True, sum_order=so, stats_order="hip")
            assert np.array_equal(q[[0, 2]], c[0][[0, 2]]) and np.array_equal(s[[0, 2]], c[2][[0, 2]])
    assert np.float16(np.float32(np.float16(1e-6)) / np.float32(127)).view(np.uint16) == 0
    (b,) = rc.flat(h)
    for so in ("hip", "reference"):
        q, scale, s, pre = fused.rms_norm_general(b.rows, g, 1e-5, with_sum=True, sum_order=so, stats_order="hip")
        for r in (0, 3):                                                       # constants that are powers of two
            assert not q[r].any() and scale[r].view(np.uint16) == 0 and s[r] == 0
        assert np.abs(q[2]).max() == 127 and scale[2] > 0                          # the spread survives a mean of 1000
    # the constant 0.1: the fp32 chain of H equal terms rounds, mean != 0.1's fp16 value, a residue below 1e-6 remains: whatever it is, it
    # is the SAME for every element, so the normalised row is constant and the int8 row holds one value
    assert len(np.unique(fused.rms_norm_general(b.rows, np.ones(h, np.float16), 1e-5, stats_order="hip")[0][1])) == 1
    # gamma = 65 504: |normalised| * 65 504 overflows fp16 wherever |normalised| > 1 - amax = scale = inf, 127 / inf = 0, int8 row 0
    huge = [x for x in rc.gammas(h) if x.notes[0]["gamma"] == "huge"][0]
    q, scale, s, _ = fused.rms_norm_general(huge.rows, huge.gamma, 1e-5, with_sum=True, sum_order="hip", stats_order="hip")
    assert not q.any() and np.isposinf(scale).all() and not np.isfinite(s).any()
    # subnormal rows: through the quantiser amax is a subnormal's fp32 value; scale = half(amax / 127) underflows to 0 or one fp16 quantum
    (sb,) = rc.subnormal(h)
    q, scale, s, _ = fused.quant_per_token(sb.rows, with_sum=True, sum_order="hip")
    assert np.abs(q[0]).max() == 127 and (scale.view(np.uint16) <= 8).all()
    assert not q[2].any() and scale[2].view(np.uint16) == 0 and s[2].view(np.uint16) == 0   # -0.0 row: amax 0, 0 * inf = NaN -> 0; +0 + -0 = +0


def test_oracle_silu_regions():
    """activation_kernels.cu:9-13 silu(x) = x / (1 + expf(-x)), rounded to half, times y: x for x >= 18, -0 for x <= -104, +-inf -> inf /
    NaN, NaN -> NaN; products beyond 65 504 are inf."""
    d = len(rc.SILU_GATES) * len(rc.SILU_UPS)
    x = rc.silu_regions(d)
    out = fused.silu_and_mul(x)[0].reshape(len(rc.SILU_GATES), len(rc.SILU_UPS))
    for (gate, region), row in zip(rc.SILU_GATES, out):
        gh = np.float16(gate)
        if region == "ge18":
            with np.errstate(over="ignore"):
                assert row[0] == gh and row[1] == -gh and row[2] == np.float16(np.float32(gh) * np.float32(300))
        elif region == "le-104":
            assert [int(v) for v in row.view(np.uint16)] == [0x8000, 0x0000, 0x8000, 0x8000]
        elif region == "subnormal":
            assert row[0] == np.float16(np.float32(gh) / 2) and row[1] == -row[0]
        elif region == "nan" or gate == -np.inf:
            assert np.isnan(row).all()
        else:
            assert np.array_equal(row, np.array([np.inf, -np.inf, np.inf, np.inf], np.float16))
    assert np.isposinf(out[[g for g, _ in rc.SILU_GATES].index(1000.0), 2])                  # 1000 * 300
