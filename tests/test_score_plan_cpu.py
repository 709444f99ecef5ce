"""The planner of qs_score_rows on the CPU (csrc/score_plan.h through qs_score_rows_plan / qs_score_rows_grid_position): the splits cover
the vocabulary's tiles exactly once, the workspace holds one 16-byte record per (padded row, split), the split count keeps its bounds,
the grid order gives every (row tile, split) to exactly one workgroup, and the entry refuses bad calls before any device call."""
import ctypes as C

import pytest

TR, TV, MAX_SPLITS = 128, 256, 64
# rows, V, K, forced splits: degenerate sizes, the test shapes of the GPU file, the Llama-3 head at 512 / 2 048 / 8 192 rows, the largest V
SHAPES = [(1, 8, 64, 0), (1, 8, 64, 5), (129, 1537, 64, 0), (5, 1537, 128, 7), (5, 1537, 128, 5), (512, 128256, 4096, 0), (2048, 128256, 4096, 0),
          (8192, 128256, 4096, 0), (8192, 128256, 8192, 1), (100000, 1 << 22, 64, 0), (1100, 3000, 64, 0)]


@pytest.fixture(scope="module")
def logprobs(built_lib):
    from qserve_amd import logprobs
    return logprobs


@pytest.mark.parametrize("rows, V, K, forced", SHAPES)
def test_splits_cover_the_vocabulary_once_and_the_workspace_matches(logprobs, rows, V, K, forced):
    p = logprobs.score_plan(rows, V, K, forced)
    assert (p["tile_rows"], p["tile_vocab"], p["depth"]) == (TR, TV, 3)
    assert p["row_tiles"] == -(-rows // TR) and p["vocab_tiles"] == -(-V // TV)
    ranges = [(s * p["tiles_per_split"], min((s + 1) * p["tiles_per_split"], p["vocab_tiles"])) for s in range(p["splits"])]
    assert [t for lo, hi in ranges for t in range(lo, hi)] == list(range(p["vocab_tiles"])) and all(lo < hi for lo, hi in ranges)
    assert 1 <= p["splits"] <= min(p["vocab_tiles"], MAX_SPLITS) and (not forced or p["splits"] <= forced)
    if not forced and p["splits"] > 1:                                     # a planned split keeps at least two tiles on average and stops at the target
        assert p["tiles_per_split"] >= 2 and (p["splits"] - 1) * p["row_tiles"] < 512
    assert p["workspace_bytes"] == 16 * p["splits"] * p["row_tiles"] * TR
    assert logprobs.lib.qs_score_rows_workspace_bytes(rows, V, K, forced) == p["workspace_bytes"]


@pytest.mark.parametrize("rows, V, K, forced", [s for s in SHAPES if s[0] <= 8192])
def test_grid_order_hands_out_every_pair_once(logprobs, rows, V, K, forced):
    p = logprobs.score_plan(rows, V, K, forced)
    grid = -(-p["row_tiles"] * p["splits"] // 8) * 8
    rt, sp, seen = C.c_int(), C.c_int(), []
    for wg in range(grid):
        if logprobs.lib.qs_score_rows_grid_position(rows, V, K, forced, wg, C.byref(rt), C.byref(sp)) == 1:
            seen.append((rt.value, sp.value))
    assert sorted(seen) == [(r, s) for r in range(p["row_tiles"]) for s in range(p["splits"])]
    assert logprobs.lib.qs_score_rows_grid_position(rows, V, K, forced, grid, C.byref(rt), C.byref(sp)) == -1


OK = dict(h=4096, hs=64, w=8192, ws=64, t=256, rows=4, V=8, K=64, lp=512, ws_ptr=16384, ws_bytes=1 << 20)


@pytest.mark.parametrize("kw, msg", [(dict(h=0), b"null pointer"), (dict(ws_ptr=0), b"null pointer"), (dict(K=96, hs=96, ws=96), b"multiple of 64"),
                                     (dict(hs=56), b"row strides"), (dict(ws=68), b"row strides"), (dict(h=4104), b"16-byte aligned"),
                                     (dict(V=7), b"n_vocab=7"), (dict(V=(1 << 22) + 1), b"n_vocab="), (dict(ws_bytes=2047), b"2048 needed")])
def test_entry_refuses_before_any_device_call(logprobs, kw, msg):
    """QS_EINVAL with a message; the addresses are never dereferenced.  rows = 0 with good arguments is QS_OK without a launch."""
    def call(**kw):
        a = {**OK, **kw}
        return logprobs.lib.qs_score_rows(a["h"], a["hs"], a["w"], a["ws"], a["t"], a["rows"], a["V"], a["K"], a["lp"], None, None, a["ws_ptr"],
                                          a["ws_bytes"], None)

    assert call(rows=0) == 0
    assert call(**kw) == -1
    err = logprobs.lib.qs_last_error()
    assert err.startswith(b"score_rows:") and msg in err, err
