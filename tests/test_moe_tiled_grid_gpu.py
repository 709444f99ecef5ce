"""The compute-bound grouped W4A8 tile (csrc/gemm_w4a8_moe_tiled.hip) where N <= 512 and 40 dense source rows never take it: grids of
more than one band of channel tiles and more than one group of row blocks (tests/_moe_tiled_cases.py; the walk and every case's geometry
are proven in tests/test_moe_tiled_grid_cpu.py), source rows beyond byte 2^31 of x, and row_src values outside [0, x_rows - 1].

Everything is bit for bit: against oracle.w4a8, against the dense entries on the gathered rows, against the streaming form, and sentinels.
A tile the walk visits twice leaves another unvisited, and that one keeps the fill; a source offset taken as signed, or a row_src used
unclamped, reads other bytes than the dense entry is given."""
import functools

import numpy as np
import pytest
import torch

import _moe_tiled_cases as cases
import test_moe_tiled_gpu as base
from oracle import synth, w4a8

pytestmark = pytest.mark.gpu
FILL = base.FILL
K = cases.K
BY_NAME = {c.name: c for c in cases.CASES}
# per_chn under the fmaf convention on the first case only: the epilogue does not depend on the grid
GRID = [(c.name, mode, epi) for i, c in enumerate(cases.CASES) for mode, epi in base.MODES if epi == 0 or i == 0]


@pytest.fixture(scope="module")
def moe(gpu):
    from qserve_amd import moe
    return moe


def _d(x, gpu):
    return torch.from_numpy(np.ascontiguousarray(x)).to(gpu)


def _lin(moe, gpu, mode, st):
    if mode == "per_chn":
        return moe.MoELinear.from_tensors(dict(qweight=_d(st["qweight"], gpu), s1_scales=_d(st["wscales"], gpu), s1_szeros=_d(st["w_szs"], gpu)), -1)
    return moe.MoELinear.from_tensors(dict(qweight=_d(st["qweight"], gpu), s1_scales=_d(st["wscales"], gpu), s2_scales=_d(st["s2_scales"], gpu),
                                           s2_zeros=_d(st["s2_zeros"], gpu)), 128)


@functools.lru_cache(maxsize=1)
def _grid_problem(mode, name):
    """A case's operands: up to eight distinct weight problems (expert e takes problem e % 8) over ONE set of 40 activation rows, the stacked
    expert tensors, and the integer accumulators of every (problem, source row) - computed once, shared by the epilogue conventions."""
    case = BY_NAME[name]
    E, N = len(case.counts), case.N
    gen = synth.per_channel_problem if mode == "per_chn" else synth.per_group_problem
    keep = ("A", "ascales", "a_ssums", "qweight", "wscales", "w_szs", "s2_scales", "s2_zeros")
    probs = [{k: v for k, v in gen(cases.X_ROWS, N, K, seed=N + e).items() if k in keep} for e in range(min(E, 8))]
    A = probs[0]["A"]
    if mode == "per_chn":
        accs = [w4a8.gemm_per_chn_acc(A, p["qweight"]) for p in probs]
    else:
        accs = [w4a8.gemm_per_group_acc(A, p["qweight"], p["s2_zeros"], p["s2_scales"]) for p in probs]
    names = ("qweight", "wscales", "w_szs") if mode == "per_chn" else ("qweight", "wscales", "s2_scales", "s2_zeros")
    return probs, {n: np.stack([probs[e % 8][n] for e in range(E)]) for n in names}, accs


def _oracle(mode, epi, probs, accs, offsets, row_src, N):
    """fp16 [P, N]: oracle.w4a8 per (expert, source row) - 40 rows per distinct problem - gathered through row_src."""
    first = probs[0]
    if mode == "per_chn":
        per = [w4a8.epilogue_per_chn(a, p["wscales"], first["ascales"], p["w_szs"], first["a_ssums"], fma=bool(epi)) for p, a in zip(probs, accs)]
    else:
        per = [w4a8.epilogue_per_group(a, p["wscales"], first["ascales"]) for p, a in zip(probs, accs)]
    want = np.empty((len(row_src), N), np.float16)
    for e in range(len(offsets) - 1):
        lo, hi = int(offsets[e]), int(offsets[e + 1])
        want[lo:hi] = per[e % 8][row_src[lo:hi]]
    return want


@pytest.mark.parametrize("name,mode,epi", GRID, ids=[f"{n}-{m}{'-epi1' if e else ''}" for n, m, e in GRID])
def test_grid_geometry(moe, gpu, name, mode, epi):
    """A case of tests/_moe_tiled_cases.py through the forced tile, rows gathered through a row_src with repeats in no order from padded
    x rows into padded out rows: the plan the case names; every element 0 ulp against the oracle; every expert bit-equal to the dense entry;
    every covered row written; rows >= P, guard columns and guard rows keep their fill; a second launch gives the same bits."""
    from qserve_amd._lib import check, lib
    case = BY_NAME[name]
    offsets, row_src = cases.routing(case)
    E, P, N = len(case.counts), len(row_src), case.N
    assert moe.gemm_tiled_plan(P, E, N, K) == (128, N // 256, case.nrb, 4)
    probs, st, accs = _grid_problem(mode, name)
    lin = _lin(moe, gpu, mode, st)
    x_store = torch.full((cases.X_ROWS, K + 16), 99, dtype=torch.int8, device=gpu)
    x_store[:, :K] = _d(probs[0]["A"], gpu)
    x, scale = x_store[:, :K], _d(probs[0]["ascales"], gpu)
    ssum = _d(probs[0]["a_ssums"], gpu) if mode == "per_chn" else None
    src, offs = _d(row_src, gpu), _d(offsets, gpu)
    stores = [torch.full((P + 3, N + 8), FILL, dtype=torch.float16, device=gpu) for _ in range(2)]
    check(lib.qs_set_gemm_epilogue(epi), "epilogue")
    try:
        for store in stores:
            moe.grouped_gemm(x, scale, ssum, offs, lin, store[:P, :N], row_src=src, form="tiled")
        base._check_against_dense(mode, lin, x, scale, ssum, src, offsets, stores[0][:P, :N], name)
    finally:
        check(lib.qs_set_gemm_epilogue(0), "epilogue")
    assert torch.equal(stores[0].view(torch.int16), stores[1].view(torch.int16)), "the second launch differs from the first"
    got = stores[0].cpu().numpy()
    del stores
    assert (got[P:] == FILL).all() and (got[:, N:] == FILL).all(), "a row >= P or a guard column was written"
    assert (got[:P, :N] != FILL).any(axis=1).all(), "a covered row was not written"
    want = _oracle(mode, epi, probs, accs, offsets, row_src, N)
    same = got[:P, :N].view(np.uint16) == want.view(np.uint16)
    if not same.all():                      # name the tiles: a wrong walk shows as whole (row block, channel tile) rectangles
        bad = sorted({(int(p) // 128, int(n) // 256) for p, n in zip(*np.nonzero(~same))})[:8]
        raise AssertionError(f"{name}: not 0 ulp against the oracle; (sorted row // 128, channel // 256) of the first differing tiles: {bad}")


FAR = (0, 1, 2047, 2048, 2049)


@pytest.mark.parametrize("mode", ["per_chn", "per_group"])
def test_far_source_rows(moe, gpu, mode):
    """x rows 2^20 bytes apart: row 2048 starts at byte 2^31 exactly, row 2049 lies beyond it, and x_rows * x_stride = 2050 * 2^20 stays
    below 2^32, so the tile must take the call with its 32-bit per-lane offsets.  Only the five rows addressed are initialised.  Both
    forms bit-equal to the dense entry on the gathered rows, and to each other."""
    E, P, N = 2, 200, 256
    offsets = np.array([0, 150, 200], np.int32)
    probs, st = base._problem(mode, E, N, K)
    lin = _lin(moe, gpu, mode, st)
    row_src = np.array(FAR, np.int32)[np.random.default_rng(P).integers(0, len(FAR), size=P)]
    assert set(row_src[:150].tolist()) == set(FAR) == set(row_src[150:].tolist())
    x_store = torch.empty((2050, 1 << 20), dtype=torch.int8, device=gpu)
    try:
        x, far = x_store[:, :K], torch.tensor(FAR, device=gpu)
        assert x.stride(0) * 2048 == 1 << 31 and x.size(0) * x.stride(0) < 1 << 32
        x[far] = _d(probs[0]["A"][:len(FAR)], gpu)
        scale = torch.zeros((2050,), dtype=torch.float16, device=gpu)
        scale[far] = _d(probs[0]["ascales"][:len(FAR)], gpu)
        ssum = None
        if mode == "per_chn":
            ssum = torch.zeros((2050,), dtype=torch.float16, device=gpu)
            ssum[far] = _d(probs[0]["a_ssums"][:len(FAR)], gpu)
        src, offs = _d(row_src, gpu), _d(offsets, gpu)
        outs = {}
        for form in ("tiled", "streaming"):
            store = torch.full((P + 3, N + 8), FILL, dtype=torch.float16, device=gpu)
            moe.grouped_gemm(x, scale, ssum, offs, lin, store[:P, :N], row_src=src, form=form)
            base._check_against_dense(mode, lin, x, scale, ssum, src, offsets, store[:P, :N], form)
            outs[form] = store.cpu().numpy()
            assert (outs[form][P:] == FILL).all() and (outs[form][:, N:] == FILL).all(), f"{form}: a row >= P or a guard column was written"
            assert (outs[form][:P, :N] != FILL).any(axis=1).all(), f"{form}: a covered row was not written"
        assert np.array_equal(outs["tiled"].view(np.uint16), outs["streaming"].view(np.uint16)), "tiled differs from streaming"
    finally:
        del x_store
        x = None
        torch.cuda.empty_cache()


@pytest.mark.parametrize("form", ["tiled", "streaming"])
@pytest.mark.parametrize("mode", ["per_chn", "per_group"])
def test_hostile_row_src(moe, gpu, mode, form):
    """row_src values below 0 and at or beyond x_rows = 40, among valid ones, in both experts' ranges: the whole buffer - results and
    sentinels - equals that of the call with the values clamped into [0, 39] on the host, which in turn equals the dense entry."""
    E, P, N, Kk = 4, 30, 256, 384
    offsets = np.array([0, 7, 7, 20, 30], np.int32)
    probs, lin, x, scale, ssum = base._setup(moe, gpu, mode, E, N, Kk)
    row_src = np.random.default_rng(7).integers(0, base.X_ROWS, size=P).astype(np.int64)
    hostile = {0: -1, 3: -(1 << 31), 6: 40, 7: (1 << 31) - 1, 12: -5, 19: 41, 20: -(1 << 31), 25: 1 << 30, 29: (1 << 31) - 1}
    for p, v in hostile.items():
        row_src[p] = v
    clamped = np.clip(row_src, 0, base.X_ROWS - 1).astype(np.int32)
    row_src = row_src.astype(np.int32)
    assert {-1, -(1 << 31), 40, (1 << 31) - 1} <= set(row_src.tolist()) and set(clamped.tolist()) >= {0, base.X_ROWS - 1}
    offs, got = _d(offsets, gpu), {}
    for what, rows in (("hostile", row_src), ("clamped", clamped)):
        store = torch.full((P + 3, N + 8), FILL, dtype=torch.float16, device=gpu)
        moe.grouped_gemm(x, scale, ssum, offs, lin, store[:P, :N], row_src=_d(rows, gpu), form=form)
        if what == "clamped":
            base._check_against_dense(mode, lin, x, scale, ssum, _d(rows, gpu), offsets, store[:P, :N], form)
        got[what] = store.cpu().numpy()
    assert np.array_equal(got["hostile"].view(np.uint16), got["clamped"].view(np.uint16)), "row_src is not clamped into [0, x_rows - 1]"
    assert (got["hostile"][P:] == FILL).all() and (got["hostile"][:, N:] == FILL).all(), "a row >= P or a guard column was written"
    assert (got["hostile"][:P, :N] != FILL).any(axis=1).all(), "a covered row was not written"
