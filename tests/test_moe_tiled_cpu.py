"""The compute-bound grouped tile without a GPU: its pure planners (`qs_moe_gemm_tiled_plan`, `qs_moe_gemm_form`) and every argument rule
the two tiled entries add to the plain ones' - each answers with a null stream, before any device call."""
import ctypes

import pytest

A16 = 4096          # a 16-byte aligned fake address


@pytest.fixture(scope="module")
def lib(built_lib):
    from qserve_amd._lib import lib
    return lib


def _call(lib, fn, P, E, N, Kk, n=4):
    out = (ctypes.c_int * n)()
    assert fn(P, E, N, Kk, out) == 0, lib.qs_last_error()
    return list(out)


def _threshold(lib, E, N, Kk):
    """The smallest rows per expert the planner gives to the tile at (N, K), or None."""
    return next((r for r in range(1, 1 << 13) if _call(lib, lib.qs_moe_gemm_form, r * E, E, N, Kk, 1) == [1]), None)


@pytest.mark.parametrize("name,counts", [("bound reached", [1] * 7 + [1000]), ("one expert", [0, 0, 777, 0]), ("uniform", [200] * 8),
                                         ("empty ends", [0, 129, 128, 1, 0]), ("64 single rows", [1] * 64)])
def test_row_block_bound_covers_the_routing(lib, name, counts):
    P, E = sum(counts), len(counts)
    rows, ntiles, rblocks, stages = _call(lib, lib.qs_moe_gemm_tiled_plan, P, E, 512, 1024)
    true_blocks = sum(-(-c // 128) for c in counts)
    assert (rows, ntiles, stages) == (128, 2, 16) and rblocks == -(-P // 128) + E - 1 and rblocks >= true_blocks
    if name in ("bound reached", "64 single rows"):
        assert rblocks == true_blocks


def test_form(lib):
    """Never tiled for N % 256 != 0, for K = 128 or below the threshold; tiled from it on; the streaming plan is what it was."""
    E = 8
    thr = _threshold(lib, E, 28672, 4096)
    assert thr is not None and thr == _threshold(lib, E, 4096, 14336) and thr > 16, "the decode step (<= 16 rows per expert) must stream"
    form = lambda P, N, Kk: _call(lib, lib.qs_moe_gemm_form, P, E, N, Kk, 1)[0]       # noqa: E731
    for r in (thr, thr + 1, 2 * thr, 2048, 16384):
        assert form(r * E, 4096, 14336) == 1 and form(r * E - E + 1, 256, 256) == 1            # ceil(P / E) = r
        assert form(r * E, 4096 + 64, 14336) == 0 and form(r * E, 4096 + 128, 14336) == 0 and form(r * E, 4096, 128) == 0
    for r in (1, 16, thr - 1):
        assert form(r * E, 4096, 14336) == 0 and form(r * E, 28672, 4096) == 0
    assert form(0, 4096, 14336) == 0
    assert form(1 << 21, 256, 1 << 12) == 0 and form(1 << 15, 256, 1 << 12) == 1               # P * K must stay below 2^32
    for P in (16, thr * E, 1 << 15):                                                             # (tests/golden/moe_plan_table.json pins the rest)
        mt = 1 if -(-P // E) <= 16 else 2 if -(-P // E) <= 32 else 4
        assert _call(lib, lib.qs_moe_gemm_plan, P, E, 4096, 14336) == [mt, 8 if mt <= 2 else 4, -(-P // (16 * mt)) + E - 1, 64]
    assert lib.qs_moe_gemm_form(16, 65, 256, 256, (ctypes.c_int * 1)()) == -1 and lib.qs_moe_gemm_form(16, 8, 256, 256, None) == -1
    assert lib.qs_moe_gemm_tiled_plan(16, 8, 320, 256, (ctypes.c_int * 4)()) == -1 and b"256" in lib.qs_last_error()
    assert lib.qs_moe_gemm_tiled_plan(16, 8, 256, 128, (ctypes.c_int * 4)()) == -1 and lib.qs_moe_gemm_tiled_plan(16, 8, 256, 256, None) == -1


@pytest.mark.parametrize("per_group", [False, True])
def test_tiled_entries_argument_rules(lib, per_group):
    ok = dict(x=A16, xs=256, xr=16, src=A16, offs=A16, qw=A16, out=A16, os=256, P=16, E=8, N=256, K=256)

    def call(**kw):
        a = dict(ok, **kw)
        if per_group:
            return lib.qs_w4a8_per_group_moe_gemm_tiled(a["x"], a["xs"], a["xr"], a["src"], a["offs"], a["qw"], A16, A16, A16, A16, a["out"], a["os"],
                                                        a["P"], a["E"], a["N"], a["K"], None)
        return lib.qs_w4a8_per_chn_moe_gemm_tiled(a["x"], a["xs"], a["xr"], a["src"], a["offs"], a["qw"], A16, A16, A16, A16, a["out"], a["os"],
                                                  a["P"], a["E"], a["N"], a["K"], None)

    added = [(dict(N=320, os=320), "multiple of 256"), (dict(N=64, os=64), "multiple of 256"), (dict(K=128, xs=128), "at least 256"),
             (dict(xr=1 << 24, xs=256), "2^32"), (dict(xr=1 << 20, xs=1 << 12, K=1 << 12), "2^32"),      # x_rows * x_stride
             (dict(N=1 << 22, os=1 << 22, K=1 << 11, xs=1 << 11), "2^32")]                               # one expert's N * K / 2
    shared = [(dict(E=65), "experts"), (dict(K=320, xs=320), "multiple of 128"), (dict(x=0), "null"), (dict(os=250), "stride"),
              (dict(src=0, xr=15), "x_rows"), (dict(qw=A16 + 4), "aligned")]                             # the plain entries' rules hold too
    for kw, word in added + shared:
        assert call(**kw) == -1 and word in lib.qs_last_error().decode(), (kw, lib.qs_last_error())
    assert call(P=0) == 0                                            # an empty call: no launch
    assert call(P=0, N=320, os=320) == -1                            # ... but still a checked one
