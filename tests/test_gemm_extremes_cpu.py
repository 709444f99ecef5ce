"""The table of tests/_gemm_extreme_cases.py, checked without a GPU: on every row's operands the oracle's accumulators equal the int64
matmul; the rows are what they claim - accumulators of at least 2^24 that fp32 cannot hold, slices that are large and cancel, the
inf / NaN layout of the overflow scales from the oracle alone; every row gets the plan it names from qs_w4a8_gemm_plan /
qs_w4a8_gemm_planes_plan / qs_moe_gemm_plan (a row that silently ran another geometry would test nothing); and every family keeps the
rows tests/test_gemm_extremes_gpu.py is there for, so a later edit cannot drop one silently."""
import ctypes as C

import numpy as np
import pytest

import _gemm_extreme_cases as cases

T24 = cases.T24
DENSE = ("own", "splitk", "pair", "tiled", "wide", "ring", "gate_up")
PROBLEMS = sorted({(r.mode, cases.source_rows(r), r.N, r.K, r.wkind, r.scales) for r in cases.TABLE}, key=str)


def _pattern_rows(M, names):
    return [i for i, p in enumerate(cases.row_patterns(M)) if p in names]


def _uniform_columns(W):
    """Columns whose weights have one value over the whole K."""
    return (W == W[:, :1]).all(axis=1)


def test_oracle_accumulators_equal_the_int64_matmul():
    seen = set()
    for key in PROBLEMS:
        if key[:5] in seen:                                            # (the scales do not enter the accumulators)
            continue
        seen.add(key[:5])
        pr = cases.problem(*key)
        exact = cases.problem_acc(*key[:5])
        if pr["A"].shape[0] <= 17 and pr["W"].size <= 1 << 21:          # the literal product where it takes no time
            assert np.array_equal(exact, pr["A"].astype(np.int64) @ pr["W"].astype(np.int64).T), key
        acc = cases.oracle_acc(pr)
        assert acc.dtype == np.int32 and np.array_equal(acc.astype(np.int64), exact), key
    zero = cases.moe_zero_expert(cases.row_problem(cases.MOE[0]))
    assert not cases.oracle_acc(zero).any()
    zero = cases.moe_zero_expert(cases.row_problem(cases.MOE[3]))
    assert not cases.oracle_acc(zero).any()


def test_operands_are_the_extremes_they_claim():
    for mode, M, N, K, wkind, scales in PROBLEMS:
        pr = cases.problem(mode, M, N, K, wkind, scales)
        A, W = pr["A"], pr["W"]
        assert A.dtype == np.int8 and A.shape == (M, K) and set(np.unique(A)) <= {-128, 126, 127}
        for i, p in enumerate(cases.row_patterns(M)):
            assert np.array_equal(A[i], cases.pattern_row(p, K))
        assert (A[_pattern_rows(M, ("neg128",))] == -128).all()
        if mode == "per_channel":
            assert W.max() == 15 and (pr["w_szs"][::16] == 0).all() and (pr["w_szs"][1::16] != 0).all()
        else:
            assert set(np.unique(W)) <= {-128, 127}
            assert (W == -128).any() == (wkind != "b127") and (W == 127).any() == (wkind != "bm128")
        assert _uniform_columns(W).any()


def test_same_sign_rows_reach_2_24_and_odd_rows_are_not_fp32_numbers():
    """Checked per case, as it must be: an `odd` row's accumulator against a weight of 127 or 15 is no multiple of the fp32 spacing at
    its magnitude (2 in [2^24, 2^25), 4 in [2^25, 2^26)) - but against -128, a power of two, it is -128 * sum A and always an fp32
    number, so an all -128 weight (bm128) carries the claim in no row and a lone `odd` row never runs against one."""
    for key in PROBLEMS:
        M, wkind = key[1], key[4]
        acc = cases.problem_acc(*key[:5])
        same = _pattern_rows(M, cases.SAME_SIGN)
        assert same and (np.abs(acc[same]).max(axis=1) >= T24).all(), key
        assert np.abs(acc).max() <= 1 << 26                             # (128 * 128 * 4096, the longest byte row)
        odd = _pattern_rows(M, ("odd",))
        assert odd, key
        for i in odd:
            big = np.abs(acc[i]) >= T24
            spacing = cases.fp32_spacing(acc[i])
            assert set(np.unique(spacing[big])) <= {2, 4, 8}
            lost = big & (acc[i] % spacing != 0)
            assert lost.any() == (wkind != "bm128") and (M > 1 or wkind != "bm128"), key
            assert (acc[i][lost].astype(np.float32).astype(np.int64) != acc[i][lost]).all()
            assert (acc[i][~lost].astype(np.float32).astype(np.int64) == acc[i][~lost]).all()


def _cancelling(pr, M):
    """Per cancel_* row: (the largest same-sign partial, |acc|) over the columns of one weight value."""
    A, W = pr["A"], pr["W"]
    rows = _pattern_rows(min(M, len(cases.PATTERNS)), ("cancel_halves", "cancel_k128", "checker"))   # (later rows repeat these)
    cols = np.flatnonzero(_uniform_columns(W) & (W[:, 0] != 0))[:8]    # (they repeat with the channel's index mod 4)
    acc = cases.exact_acc(A[rows], W[cols])
    pos = cases.exact_acc(np.maximum(A[rows], 0), W[cols])             # the slices with A > 0: a half, every other k-step or element
    return rows, np.maximum(np.abs(pos), np.abs(acc - pos)), np.abs(acc)


def test_cancelling_rows_have_large_partials_and_a_small_total():
    """Halves (cancel_halves), every other 128-step (cancel_k128) and every other element (checker) are same-sign partials.  Byte rows
    from K = 2176 on: a partial of at least 2^24 and a total below it.  Per-channel rows and K = 1152 ... 2048 cannot reach that (the
    whole sum of |a w| stays below 2^25): their largest partial is at least 2^23 there.  Everywhere the total is at most a quarter of
    the partial (an odd number of k-steps leaves one step's worth over)."""
    for key in PROBLEMS:
        pr = cases.problem(*key)
        mode, M, K = key[0], key[1], key[3]
        if M < 3:
            continue
        rows, partial, total = _cancelling(pr, M)
        claim = T24 if mode != "per_channel" and K >= 2176 else T24 // 2
        assert (partial.min(axis=1) >= claim).all(), (key, partial.min())
        assert (total.max(axis=1) < T24).all() and (total * 4 <= partial).all(), key
        if M >= 6:
            assert {cases.row_patterns(M)[i] for i in rows} == {"cancel_halves", "cancel_k128", "checker"}


def test_overflow_scales_give_inf_and_nan_from_the_oracle_alone():
    """ascales = 0.05 at K = 14 336: a_ssums of the same-sign rows is +-inf, so the columns with w_sz = 0 (z = 0) are NaN and the others
    inf of the sign of -a_ssums; the cancelling rows and the whole finite set stay finite.  Both epilogue conventions."""
    seen = 0
    for key in PROBLEMS:
        mode, M, N, K, wkind, scales = key
        if mode != "per_channel" or scales == "tie":
            continue
        pr = cases.problem(*key)
        acc = cases.oracle_acc(pr)
        same = _pattern_rows(M, cases.SAME_SIGN)
        other = [i for i in range(M) if i not in same]
        for fma in (False, True):
            out = cases.oracle_out(pr, acc, fma=fma)
            assert np.isfinite(out[other]).all(), key
            if scales == "finite":
                assert np.isfinite(pr["a_ssums"]).all() and np.abs(pr["a_ssums"]).max() <= 55040 and np.isfinite(out).all(), key
                continue
            assert K == 14336 and np.isinf(pr["a_ssums"][same]).all() and np.isfinite(pr["a_ssums"][other]).all(), key
            zero = pr["w_szs"] == 0
            assert zero.any() and np.array_equal(zero, pr["z"] == 0)
            assert np.isnan(out[same][:, zero]).all() and np.isinf(out[same][:, ~zero]).all(), key
            assert (np.sign(out[same][:, ~zero]) == -np.sign(pr["a_ssums"][same])[:, None]).all(), key
            seen += 1
    assert seen


def test_tie_scales_make_the_fp16_output_see_the_conversion():
    """With constant scales the 11 significant bits of an fp16 output mostly hide how the epilogue rounds (float)acc.  Under the `tie`
    scales outputs change in every problem, under both per-channel conventions: of the `odd3` rows when (float)acc truncates -
    other_fp32 is the truncated value there, (float)acc rounds those away from zero - and of the `odd` rows when it rounds a tie away
    from zero.  So the fp16 comparisons on the GPU fail for a kernel whose epilogue converts differently."""
    def truncated(v):
        f = v.astype(np.float32)
        return np.where(np.abs(f.astype(np.int64)) > np.abs(v), np.nextafter(f, np.float32(0)), f).astype(np.float32)

    for key in PROBLEMS:
        mode, M, N, K, wkind, scales = key
        if scales != "tie":
            continue
        pr = cases.problem(*key)
        acc = cases.problem_acc(*key[:5])
        for pattern in ("odd", "odd3"):
            rows = _pattern_rows(min(M, len(cases.PATTERNS)), (pattern,))
            if not rows:
                continue
            near, other = acc[rows].astype(np.float32), cases.other_fp32(acc[rows])
            lost = near != other
            assert np.array_equal(truncated(acc[rows])[lost], (other if pattern == "odd3" else near)[lost]), key
            sub = dict(pr, ascales=pr["ascales"][rows])
            if mode == "per_channel":
                sub["a_ssums"] = pr["a_ssums"][rows]
            for fma in (False, True) if mode == "per_channel" else (False,):
                outs = [cases.oracle_out(sub, v, fma=fma) for v in (near, other)]
                assert np.isfinite(outs[0]).all() and np.isfinite(cases.oracle_out(pr, acc, fma=fma)).all(), key
                assert (outs[0].view(np.uint16) != outs[1].view(np.uint16)).any(), (key, pattern, fma)
    assert any(k[5] == "tie" and k[1] >= 7 for k in PROBLEMS)


@pytest.fixture(scope="module")
def lib(built_lib):
    from qserve_amd._lib import lib
    return lib


def _planned(lib, row):
    from qserve_amd._lib import check
    per_group = int(row.mode != "per_channel")
    if row.family == "moe":
        buf = (C.c_int * 4)()
        check(lib.qs_moe_gemm_plan(row.M, len(row.extra), row.N, row.K, buf), "moe gemm plan")
        return tuple(buf)
    buf = (C.c_int * (4 if row.family == "planes" else 5))()
    lib.qs_set_gemm_variant(row.code)
    try:
        fn = lib.qs_w4a8_gemm_planes_plan if row.family == "planes" else lib.qs_w4a8_gemm_plan
        check(fn(per_group, row.M, row.N, row.K, C.cast(buf, C.c_void_p)), "w4a8 gemm plan")
    finally:
        lib.qs_set_gemm_variant(-1)
    return tuple(buf)


def test_every_row_plans_as_it_claims(lib):
    for row in cases.TABLE:
        if row.family == "w8a8":                                        # one kernel, no planner: only the shapes it takes
            assert row.plan is None and row.N % 16 == 0 and row.K % 64 == 0
            continue
        got = _planned(lib, row)
        assert len(got) == len(row.plan) and all(w is None or w == g for w, g in zip(row.plan, got)), (cases.row_id(row), got)
        if row.family in DENSE and row.family != "own" and row.family != "gate_up":
            want = {"splitk": cases.F_SPLITK, "pair": cases.F_PAIR, "tiled": cases.F_TILED, "wide": cases.F_WIDE, "ring": cases.F_RING}
            assert row.plan[0] == want[row.family], cases.row_id(row)
        if row.family in ("ring", "planes") and row.code >= 0:
            assert cases.ring_fits(row.code, row.N, row.K), cases.row_id(row)
        if row.family == "planes":
            assert got[0] in (1, 2, 4) and (row.code < 0 or got[0] == cases.ring_geometry(row.code)[2])
        if row.family == "moe":
            assert sum(row.extra) == row.M and got[3] == row.N // 64


def test_sizes_stay_inside_the_limits_and_say_where_k_was_substituted():
    assert len({cases.row_id(r) for r in cases.TABLE}) == len(cases.TABLE)
    for row in cases.TABLE:
        assert 1 <= row.M <= 130 and row.N <= 512 and row.K <= 14336 and row.K % 128 == 0, cases.row_id(row)
        listed = cases.PC_K if row.mode == "per_channel" else cases.BYTE_K
        assert (row.K in listed) == (not row.note.startswith("K ")), cases.row_id(row)
        assert row.K >= listed[0], "every K reaches 2^24"
        if row.scales == "overflow":
            assert row.mode == "per_channel" and row.K == 14336


def test_every_family_keeps_its_rows():
    """Per family: an accumulator of at least 2^24 that fp32 cannot hold (every row has an `odd` activation row: checked above on every
    problem), a neg128 row, a cancel_* row - for the byte modes one whose partials reach 2^24 - and, for the families with a
    per-channel epilogue, an overflow-set row."""
    assert {r.family for r in cases.TABLE} == set(cases.FAMILIES)
    for fam in cases.FAMILIES:
        rows = [r for r in cases.TABLE if r.family == fam]
        assert all(r.wkind != "bm128" or cases.source_rows(r) > 1 for r in rows)   # `odd` is row 0; not against -128 alone
        assert any(r.wkind != "bm128" and r.mode != "per_channel" for r in rows), f"{fam}: no byte row that fp32 cannot hold"
        assert any(cases.source_rows(r) >= 2 for r in rows), f"{fam}: no neg128 row"
        assert any(cases.source_rows(r) >= 6 and r.mode != "per_channel" and r.K >= 2176 for r in rows), f"{fam}: no cancelling row beyond 2^24"
        if fam != "w8a8":
            assert any(cases.source_rows(r) >= 6 and r.mode == "per_channel" for r in rows), f"{fam}: no per-channel cancelling row"
            assert any(r.scales == "overflow" and cases.source_rows(r) >= 4 for r in rows), f"{fam}: no overflow-set row"
            assert {r.mode for r in rows} >= {"per_channel", "per_group"}
        assert {r.mode == "per_channel" for r in rows if r.scales == "tie"} == ({False} if fam == "w8a8" else {False, True}), f"{fam}: no tie-scale row"
        assert {r.K for r in rows if r.mode != "per_channel"} & {1152, 1280, 1536, 2048} and any(r.K >= 2176 for r in rows if r.mode != "per_channel")
    # the forced families, geometry by geometry
    import _gemm_family_cases as family
    assert {r.plan[2] for r in cases.SPLITK if r.plan[3] == 1} == {1, 2, 4, 8} == {r.plan[2] for r in cases.SPLITK if r.plan[3] > 1}
    assert {(r.code, r.M, r.N, r.plan[1:]) for r in cases.SPLITK} <= {(family.splitk_code(*s[:3]), s[3], s[4], s[6]) for s in family.SPLITK}
    for code, M, N in cases._RING:
        assert {r.mode for r in cases.RING if r.code == code} == set(cases.MODES)
    assert any(r.plan[4] == 2 and r.N // (64 * r.plan[2]) % 4 == 0 for r in cases.RING), "a two-slice seam that takes the XCD mapping"
    assert {cases.ring_geometry(r.code)[2] for r in cases.RING} == {1, 2, 4} == {r.plan[0] for r in cases.PLANES}
    assert {r.extra for r in cases.MOE} == {(20, 13), (7, 3), (70, 40)} and {r.plan[0] for r in cases.MOE} == {1, 2, 4}
    offsets, row_src = cases.moe_routing(cases.MOE[0])
    assert offsets.tolist() == [0, 20, 33] and len(set(row_src.tolist())) < len(row_src) and (np.diff(row_src) < 0).any()
