"""The case tables of tests/_gemm_family_cases.py, checked without a GPU: every row of the split-K and LDS-pair sweeps gets
exactly the plan it claims from qs_w4a8_gemm_plan under its selection code (the planner clamps codes and the pair kernel takes
precedence at some shapes - a sweep over rows that silently ran another geometry would be vacuous), and the tables cover the
instantiations, wave counts, K ranges and grid mappings tests/test_gemm_decode_families_gpu.py is there for."""
import ctypes as C

import pytest

import _gemm_family_cases as cases


@pytest.fixture(scope="module")
def plan(built_lib):
    """(M, N, K, per_group, code) -> (family, p0, p1, p2, p3) as the built library plans it; the code is reset afterwards."""
    from qserve_amd._lib import check, lib

    def plan_of(M, N, K, per_group, code):
        buf = (C.c_int * 5)()
        lib.qs_set_gemm_variant(code)
        try:
            check(lib.qs_w4a8_gemm_plan(int(per_group), M, N, K, C.cast(buf, C.c_void_p)), "w4a8 gemm plan")
        finally:
            lib.qs_set_gemm_variant(-1)
        return tuple(buf)
    return plan_of


def test_split_k_rows_plan_as_they_claim(plan):
    for row in cases.SPLITK:
        mo, S, NW, M, N, K, want = row
        assert N <= 1024 and M <= 200, "the pair kernel must not be able to take a split-K row"
        for per_group in (False, True):
            got = plan(M, N, K, per_group, cases.splitk_code(mo, S, NW))
            assert got == (cases.FAMILY_SPLITK,) + want, (row, per_group, got)


def test_pair_rows_plan_as_pair(plan):
    for M, N, K in cases.PAIR:
        for per_group in (False, True):
            assert plan(M, N, K, per_group, cases.PAIR_FORCED)[0] == cases.FAMILY_PAIR, (M, N, K, per_group)
    for M, N, K in cases.PAIR_PREFILL:
        for per_group in (False, True):
            assert plan(M, N, K, per_group, -1)[0] == cases.FAMILY_PAIR, (M, N, K, per_group)


def test_dispatchers_own_route_at_small_shapes(plan):
    """Code -1: the production paths into the two kernels, at shapes small enough for the oracle."""
    for (M, N, K), want in cases.OWN_ROUTE:
        for per_group in (False, True):
            got = plan(M, N, K, per_group, -1)
            assert all(w is None or w == g for w, g in zip(want, got)), ((M, N, K), per_group, got)
    assert set(cases.PAIR_PREFILL) <= {shape for shape, _ in cases.OWN_ROUTE}


def test_epilogue_convention_rows_plan_as_they_claim(plan):
    for code, M, N, K, want in cases.EPILOGUE_FMA:
        got = plan(M, N, K, False, code)
        assert all(w is None or w == g for w, g in zip(want, got)), (code, M, N, K, got)
    assert any(w[0] == cases.FAMILY_PAIR and cases.pair_m_tiles(M) < 4 for _, M, _, _, w in cases.EPILOGUE_FMA)
    assert any(w[0] == cases.FAMILY_SPLITK and w[3] > 1 for _, _, _, _, w in cases.EPILOGUE_FMA)


def test_cross_block_rows_cannot_fall_back_for_lack_of_space():
    """The launcher runs S = 1 when the slabs or the counters of a launch do not fit the workspace."""
    split = [r for r in cases.SPLITK if r[6][2] > 1]
    assert split
    for row in split:
        gx, gy = cases.splitk_grid(row)
        assert cases.splitk_slab_bytes(row) <= cases.SLAB_BYTES and gx * gy < cases.MAX_TILES, row


def test_split_k_table_covers_the_kernel():
    rows = cases.SPLITK
    plans = [r[6] for r in rows]
    # 4 m-tile counts x 2 modes x 2 output kinds = the 16 instantiations (every row runs in every mode and both output kinds)
    assert len(cases.MODES) == 3 and len({(p[0], mode > 0, outk) for p in plans for mode in range(3) for outk in range(2)}) == 16
    # every (m-tiles, waves) pair the clamp allows, un-split and cross-block
    allowed = {(mt, nw) for mt in (1, 2, 3, 4) for nw in (1, 2, 4, 8) if nw <= (8 if mt <= 2 else 4)}
    assert {(p[0], p[1]) for p in plans if p[2] == 1} == allowed
    assert {(p[0], p[1]) for p in plans if p[2] > 1} == allowed
    # every override x wave-count code, un-split and cross-block
    codes = {(mo, nw) for mo in (1, 2, 3, 4, 9) for nw in (1, 2, 4, 8)}
    assert codes <= {(r[0], r[2]) for r in rows if r[1] == 1} and codes <= {(r[0], r[2]) for r in rows if r[1] > 1}
    assert {p[2] for p in plans} == {1, 2, 3, 4}
    # the clamps themselves: every one of them changes some row's code
    assert any(r[2] == 8 and r[6][1] == 4 and r[5] // 128 >= 8 for r in rows), "8 waves -> 4 at m_tiles > 2"
    assert {r[2] for r in rows if r[6][1] == 4 and r[2] != 4} >= {3, 5, 6, 7}
    assert any(r[2] > r[5] // 128 and r[6][1] == 1 for r in rows), "waves > K/128 -> 1"
    # the shapes of the sweep
    assert {r[5] for r in rows} == {128, 384, 640, 1664, 2176}
    assert {r[3] for r in rows} == {1, 16, 17, 33, 50, 64, 65, 130}
    assert {r[4] for r in rows} == {64, 192, 512}
    # cross-block K ranges: a block with nothing to do, uneven ranges, and the two named in the kernel's notes
    steps = {(r[5] // 128, r[6][2]): cases.splitk_block_steps(r) for r in rows if r[6][2] > 1}
    assert all(sum(s) == n for (n, _), s in steps.items())
    assert any(0 in s for s in steps.values()), "S > K/128"
    assert steps[(3, 4)] == [0, 1, 1, 1] and steps[(5, 3)] == [1, 2, 2]
    # 8 waves x 2 stages: a partial first round (13 steps) and a second round with one live wave (17)
    assert {r[5] // 128 for r in rows if r[6][1] == 8 and r[6][2] == 1} >= {13, 17}
    # XCD flag with several token blocks: taken over 8 units, silently dropped over 3 and for S > 1
    flagged = [r for r in rows if r[6][3] == 1 and cases.splitk_grid(r)[1] > 1]
    assert any(cases.splitk_runs_xcd_mapping(r) for r in flagged)
    assert any(r[4] // 64 % 8 != 0 and not cases.splitk_runs_xcd_mapping(r) for r in flagged)
    assert any(r[4] // 64 % 8 == 0 and r[6][2] > 1 and not cases.splitk_runs_xcd_mapping(r) for r in flagged)
    assert max(cases.splitk_grid(r)[1] for r in rows if cases.splitk_runs_xcd_mapping(r)) == 9


def test_pair_table_covers_the_kernel():
    rows = cases.PAIR
    assert len({(cases.pair_m_tiles(M), mode > 0, outk) for M, _, _ in rows for mode in range(3) for outk in range(2)}) == 16
    assert {K // 128 for _, _, K in rows} == {2, 3, 5, 9, 16}
    assert {cases.pair_local_steps(K) for _, _, K in rows} == {(1, 1), (1, 2), (2, 3), (4, 5), (8, 8)}
    assert {M for M, _, _ in rows} == {1, 16, 23, 32, 40, 48, 50, 64, 65, 200}
    assert {N for _, N, _ in rows} == {128, 384}
    # every m-tile count meets an odd number of k-steps (uneven halves) and three channel blocks
    for mt in (1, 2, 3, 4):
        assert any(cases.pair_m_tiles(M) == mt and K // 128 % 2 == 1 for M, _, K in rows), mt
        assert any(cases.pair_m_tiles(M) == mt and N == 384 for M, N, _ in rows), mt
    # several token blocks x three channel blocks x uneven halves: the start rotation differs along both grid axes
    assert any(M > 64 and N == 384 and K // 128 % 2 == 1 for M, N, K in rows)


def test_w8a8_table_leaves_idle_waves_and_ragged_blocks():
    assert {cases.w8a8_idle_waves(N) for _, N, _ in cases.W8A8} >= {0, 2, 3}
    assert any(M % 64 for M, _, _ in cases.W8A8) and any(M % 64 == 0 for M, _, _ in cases.W8A8) and any(M > 64 for M, _, _ in cases.W8A8)
    assert all(N % 16 == 0 and K % 64 == 0 for _, N, K in cases.W8A8)
