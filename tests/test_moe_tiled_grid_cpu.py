"""tests/_moe_tiled_cases.py, checked without a GPU: the restated block -> (row block, channel tile) walk of the grouped tile is a
bijection onto the grid for every size up to 50 x 50, and every case has the bands, groups and surplus row blocks it names - with the
tile's sizes and the row-block bound taken from qs_moe_gemm_tiled_plan, so a case cannot silently become one band when the tile changes."""
import ctypes as C

import numpy as np
import pytest

import _moe_tiled_cases as cases


@pytest.fixture(scope="module")
def lib(built_lib):
    from qserve_amd._lib import lib
    return lib


def _plan(lib, P, E, N, K):
    from qserve_amd._lib import check
    buf = (C.c_int * 4)()
    check(lib.qs_moe_gemm_tiled_plan(P, E, N, K, buf), "moe gemm tiled plan")
    return tuple(buf)


def test_walk_is_a_bijection_onto_the_grid():
    for nrb in range(1, 51):
        for nbn in range(1, 51):
            seen = {cases.walk(b, nrb, nbn) for b in range(nrb * nbn)}
            assert seen == {(bm, bn) for bm in range(nrb) for bn in range(nbn)}, (nrb, nbn)


def test_walk_runs_row_blocks_fastest_inside_bands_and_groups():
    """The order itself, on a grid with a partial band and a partial group: ids of a band are consecutive, inside it those of a group,
    inside a group a channel tile's row blocks."""
    nrb, nbn = 19, 21
    order = [cases.walk(b, nrb, nbn) for b in range(nrb * nbn)]
    assert order[:3] == [(0, 0), (1, 0), (2, 0)] and order[16] == (0, 1) and order[16 * 16] == (16, 0)
    assert order[16 * 16 + 3] == (16, 1) and order[nrb * 16] == (0, 16) and order[nrb * 16 + 16] == (0, 17)
    assert order[nrb * 16 + 16 * 5] == (16, 16) and order[-1] == (18, 20)
    bands = [bn // cases.BAND for _, bn in order]
    assert bands == sorted(bands)
    for band in set(bands):
        groups = [bm // cases.GROUP for bm, bn in order if bn // cases.BAND == band]
        assert groups == sorted(groups)


@pytest.mark.parametrize("case", cases.CASES, ids=[c.name for c in cases.CASES])
def test_case_has_the_geometry_it_claims(lib, case):
    E, P = len(case.counts), sum(case.counts)
    rows, ntiles, nrb, stages = _plan(lib, P, E, case.N, cases.K)
    assert case.N % ntiles == 0 and _plan(lib, P, E, case.N // ntiles, cases.K)[1] == 1      # N / ntiles = the channels of one tile
    assert stages == 4 and nrb == case.nrb and E <= 64
    assert cases.geometry(nrb, ntiles) == (case.bands, case.width, case.groups, case.height)
    assert nrb - cases.true_blocks(case.counts, rows) == case.surplus >= 0
    offsets, row_src = cases.routing(case)
    assert offsets.tolist() == np.concatenate([[0], np.cumsum(case.counts)]).tolist() and row_src.shape == (P,)
    assert row_src.min() >= 0 and row_src.max() < cases.X_ROWS
    assert len(set(row_src.tolist())) < P and (np.diff(row_src) < 0).any()                   # repeats, no order
    # every band and every group of the case is entered: the walk's images, band by band and group by group
    image = {cases.walk(b, nrb, ntiles) for b in range(nrb * ntiles)}
    assert len(image) == nrb * ntiles
    assert {(bm // cases.GROUP, bn // cases.BAND) for bm, bn in image} == {(g, b) for g in range(case.groups) for b in range(case.bands)}


def test_cases_reach_what_the_issue_names(lib):
    """Between them: more than one band, a band one tile wide, a partial band wider than that, an exact band; a group one block high
    behind full ones, a partial group higher than that, full groups only; surplus row blocks; an empty expert and one-row experts."""
    by = {c.name: c for c in cases.CASES}
    assert len(by) == len(cases.CASES) == 4
    assert {c.bands for c in cases.CASES} == {1, 2, 3} and {c.width for c in cases.CASES} == {1, 4, 16}
    assert {c.groups for c in cases.CASES} == {1, 2, 3} and {c.height for c in cases.CASES} == {1, 3, 16}
    assert by["three_bands_ragged"].surplus == 2 and 0 in by["three_bands_ragged"].counts and by["three_bands_ragged"].counts[-1] == 1
    assert by["full_band_partial_groups"].counts.count(1) == 24
    rows = _plan(lib, 1, 1, 256, cases.K)[0]
    assert by["band_plus_one"].counts == (16 * rows + 1,) and by["partial_band_full_group"].counts == (16 * rows,)
