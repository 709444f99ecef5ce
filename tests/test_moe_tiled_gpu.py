"""The compute-bound grouped W4A8 tile (csrc/gemm_w4a8_moe_tiled.hip) on the GPU, through the forced entries (`form="tiled"`): bit-equal
to the dense entries per expert, 0 ulp against oracle.w4a8 at one routing per mode, and to the streaming form where the planner takes the
tile by itself.  The ring is 6 stages of 64 k deep: K = 256 fills less than it, 384 exactly it, 1024 wraps it; test_tiled_stage_counts runs every even
stage count between.  Grids wider than two channel tiles, far source rows and hostile row_src: tests/test_moe_tiled_grid_gpu.py; extreme
operands: the moe_tiled family of tests/test_gemm_extremes_gpu.py."""
import functools

import numpy as np
import pytest
import torch

from oracle import synth, w4a8

pytestmark = pytest.mark.gpu
X_ROWS = 40
FILL = float(np.float16(-1234.0))
MODES = [("per_chn", 0), ("per_chn", 1), ("per_group", 0)]
MODE_IDS = ["per_chn-epi0", "per_chn-epi1", "per_group"]
# rows per expert: a one-row tile with empty experts at either end; exactly one tile, one row over, one short around an empty expert; one
# expert over three blocks; the grid bound reached by 64 tiles of one row
ROUTINGS = {"first": [1, 0, 0, 0], "last": [0, 0, 0, 1], "edges": [128, 0, 129, 127], "one-expert": [300], "64x1": [1] * 64}


@pytest.fixture(scope="module")
def moe(gpu):
    from qserve_amd import moe
    return moe


@functools.lru_cache(maxsize=None)
def _problem(mode, E, N, Kk):
    """E experts' weights (oracle.synth; eight distinct problems, expert e takes problem e % 8) over ONE set of X_ROWS activation rows."""
    base = [(synth.per_channel_problem if mode == "per_chn" else synth.per_group_problem)(X_ROWS, N, Kk, seed=N + Kk + e) for e in range(min(E, 8))]
    probs = [base[e % 8] for e in range(E)]
    names = ("qweight", "wscales", "w_szs") if mode == "per_chn" else ("qweight", "wscales", "s2_scales", "s2_zeros")
    return probs, {n: np.stack([p[n] for p in probs]) for n in names}


def _setup(moe, gpu, mode, E, N, Kk):
    probs, st = _problem(mode, E, N, Kk)
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(gpu)       # noqa: E731
    if mode == "per_chn":
        lin = moe.MoELinear.from_tensors(dict(qweight=d(st["qweight"]), s1_scales=d(st["wscales"]), s1_szeros=d(st["w_szs"])), -1)
    else:
        lin = moe.MoELinear.from_tensors(dict(qweight=d(st["qweight"]), s1_scales=d(st["wscales"]), s2_scales=d(st["s2_scales"]),
                                              s2_zeros=d(st["s2_zeros"])), 128)
    x_store = torch.full((X_ROWS, Kk + 16), 99, dtype=torch.int8, device=gpu)      # padded rows
    x_store[:, :Kk] = d(probs[0]["A"])
    return probs, lin, x_store[:, :Kk], d(probs[0]["ascales"]), d(probs[0]["a_ssums"]) if mode == "per_chn" else None


def _dense(mode, lin, e, x, scale, ssum):
    """The dense entry on expert e's tensors and these (contiguous) rows."""
    import qserve_backend.qgemm_w4a8_per_chn as gemm_chn
    import qserve_backend.qgemm_w4a8_per_group as gemm_grp
    out, w = torch.empty((x.size(0), lin.n), dtype=torch.float16, device=x.device), lin.expert(e)
    if mode == "per_chn":
        gemm_chn.gemm_forward_cuda(x, w["qweight"], w["s1_scales"], scale, w["s1_szeros"], ssum, out)
    else:
        gemm_grp.gemm_forward_cuda(x, w["qweight"], w["s2_zeros"], w["s2_scales"], w["s1_scales"], scale, out)
    return out


def _check_against_dense(mode, lin, x, scale, ssum, src, bounds, out, what):
    for e in range(lin.experts):
        lo, hi = max(0, min(int(bounds[e]), out.size(0))), max(0, min(int(bounds[e + 1]), out.size(0)))
        if hi <= lo:
            continue
        rows = src[lo:hi].long()
        want = _dense(mode, lin, e, x[rows].contiguous(), scale[rows].contiguous(), ssum[rows].contiguous() if ssum is not None else None)
        assert torch.equal(want.view(torch.int16), out[lo:hi].contiguous().view(torch.int16)), f"{what}: expert {e} differs from the dense op"


@pytest.mark.parametrize("routing", list(ROUTINGS))
@pytest.mark.parametrize("N", [256, 512])
@pytest.mark.parametrize("Kk", [256, 384, 1024])
@pytest.mark.parametrize("mode,epi", MODES, ids=MODE_IDS)
def test_tiled_against_dense(moe, gpu, mode, epi, Kk, N, routing):
    """The forced tile, rows gathered through a row_src with repeats in no order from padded x rows into padded out rows: bit-equal to the
    dense entry per expert; rows >= P and the guard columns keep their fill; "edges" also 0 ulp against the oracle pair by pair."""
    _tiled_against_dense(moe, gpu, mode, epi, Kk, N, routing)


@pytest.mark.parametrize("Kk", [512, 640, 768, 896])
@pytest.mark.parametrize("mode,epi", MODES, ids=MODE_IDS)
def test_tiled_stage_counts(moe, gpu, mode, epi, Kk):
    """With K = 256 and 384 above, every even stage count nh = K / 64 from 4 to 14 around the ring's depth of 6: the steady loop runs 1, 2,
    3 and 4 times before the drain, and the run-time wait counts of fill and drain take each of their values.  The assertions of
    test_tiled_against_dense on "edges", the 0-ulp oracle included."""
    _tiled_against_dense(moe, gpu, mode, epi, Kk, 256, "edges")


def _tiled_against_dense(moe, gpu, mode, epi, Kk, N, routing):
    from qserve_amd._lib import check, lib
    counts = ROUTINGS[routing]
    E, P = len(counts), sum(counts)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    row_src = np.random.default_rng(Kk + N + P).integers(0, X_ROWS, size=P).astype(np.int32)
    assert moe.gemm_tiled_plan(P, E, N, Kk) == (128, N // 256, -(-P // 128) + E - 1, Kk // 64)
    probs, lin, x, scale, ssum = _setup(moe, gpu, mode, E, N, Kk)
    src = torch.from_numpy(row_src).to(gpu)
    out_store = torch.full((P + 3, N + 8), FILL, dtype=torch.float16, device=gpu)
    check(lib.qs_set_gemm_epilogue(epi), "epilogue")
    try:
        moe.grouped_gemm(x, scale, ssum, torch.from_numpy(offsets).to(gpu), lin, out_store[:P, :N], row_src=src, form="tiled")
        _check_against_dense(mode, lin, x, scale, ssum, src, offsets, out_store[:P, :N], routing)
    finally:
        check(lib.qs_set_gemm_epilogue(0), "epilogue")
    got = out_store.cpu().numpy()
    assert (got[P:] == FILL).all() and (got[:, N:] == FILL).all(), "a row >= P or a guard column was written"
    if routing != "edges":
        return
    for e in range(E):
        rows, p = row_src[offsets[e]:offsets[e + 1]], probs[e]
        if rows.size == 0:
            continue
        if mode == "per_chn":
            want = w4a8.epilogue_per_chn(w4a8.gemm_per_chn_acc(probs[0]["A"][rows], p["qweight"]), p["wscales"], probs[0]["ascales"][rows],
                                         p["w_szs"], probs[0]["a_ssums"][rows], fma=bool(epi))
        else:
            want = w4a8.gemm_per_group(probs[0]["A"][rows], p["qweight"], p["s2_zeros"], p["s2_scales"], p["wscales"], probs[0]["ascales"][rows])[1]
        assert np.array_equal(got[offsets[e]:offsets[e + 1], :N].view(np.uint16), want.view(np.uint16)), f"expert {e}: not 0 ulp against the oracle"


@pytest.mark.parametrize("mode,epi", MODES[::2], ids=MODE_IDS[::2])
@pytest.mark.parametrize("case", ["permuted", "null", "hostile"])
def test_row_sources_and_offsets(moe, gpu, mode, epi, case):
    """permuted: row_src a permutation of the P sorted rows' sources with repeats, x_rows = 40 > P = 30.  null: no row_src, x row p.
    hostile: offsets negative, beyond P and running backwards - the clamped ranges leave only expert 2 with rows 10 .. 29; those are
    bit-equal, every other element of the buffer keeps its fill."""
    E, P, N, Kk = 4, 30, 256, 384
    probs, lin, x, scale, ssum = _setup(moe, gpu, mode, E, N, Kk)
    offsets = np.array([25, 10, 10, 9999, -3] if case == "hostile" else [0, 7, 7, 20, 30], np.int32)
    perm = np.random.default_rng(3).permutation(np.arange(P) // 2 + 20).astype(np.int32)      # sources 20 .. 34, each twice, shuffled
    src = torch.arange(P, dtype=torch.int32, device=gpu) if case == "null" else torch.from_numpy(perm).to(gpu)
    out_store = torch.full((P + 3, N + 8), FILL, dtype=torch.float16, device=gpu)
    moe.grouped_gemm(x, scale, ssum, torch.from_numpy(offsets).to(gpu), lin, out_store[:P, :N], row_src=None if case == "null" else src,
                     form="tiled")
    _check_against_dense(mode, lin, x, scale, ssum, src, offsets, out_store[:P, :N], case)
    got = out_store.cpu().numpy()
    covered = slice(10, 30) if case == "hostile" else slice(0, P)
    assert (got[covered, :N] != FILL).any(axis=1).all(), "a covered row was not written"
    got[covered, :N] = FILL
    assert (got == FILL).all(), "an element outside the covered rows was written"


@pytest.mark.parametrize("mode,epi", MODES[::2], ids=MODE_IDS[::2])
def test_planner_choice_equals_streaming(moe, gpu, mode, epi):
    """At the smallest P the planner gives to the tile (E = 1, N = 256, K = 256), the plain call and the forced streaming form give equal
    bits."""
    E, N, Kk = 1, 256, 256
    P = next(p for p in (1 << i for i in range(5, 17)) if moe.gemm_form(p, E, N, Kk) == "tiled")
    assert moe.gemm_form(P // 2, E, N, Kk) == "streaming" or P == 32
    probs, lin, x, scale, ssum = _setup(moe, gpu, mode, E, N, Kk)
    src = torch.from_numpy(np.random.default_rng(P).integers(0, X_ROWS, size=P).astype(np.int32)).to(gpu)
    offs = torch.tensor([0, P], dtype=torch.int32, device=gpu)
    a, b = (torch.full((P, N), FILL, dtype=torch.float16, device=gpu) for _ in range(2))
    moe.grouped_gemm(x, scale, ssum, offs, lin, a, row_src=src)
    moe.grouped_gemm(x, scale, ssum, offs, lin, b, row_src=src, form="streaming")
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    _check_against_dense(mode, lin, x, scale, ssum, src, [0, P], a, "auto")
