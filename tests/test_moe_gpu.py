"""The mixture-of-experts kernels on the GPU: qs_moe_route against the restatement of tests/_moe_cases.py, the grouped W4A8 GEMMs at 0 ulp
against oracle.w4a8 and bit-equal to the dense entries per expert, qs_moe_combine bit-equal to its restatement."""
import numpy as np
import pytest
import torch

import _moe_cases as K
from oracle import synth, w4a8

pytestmark = pytest.mark.gpu
CASES = K.route_cases()
GUARD = 16


@pytest.fixture(scope="module")
def moe(gpu):
    from qserve_amd import moe
    return moe


def _guarded(shape, dtype, dev, fill):
    """A contiguous tensor of `shape` inside a larger buffer filled with `fill`: (buffer, view)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev)
    return buf, buf[GUARD:GUARD + n].view(shape)


def _untouched(buf, fill, what):
    assert (buf[:GUARD] == fill).all() and (buf[-GUARD:] == fill).all(), f"{what}: a guard element was written"


def _route(moe, logits, k, dev):
    T, E = logits.shape
    bufs = [_guarded((T, k), torch.int32, dev, -77), _guarded((T, k), torch.float32, dev, -5.0), _guarded((E + 1,), torch.int32, dev, -77),
            _guarded((T * k,), torch.int32, dev, -77), _guarded((T, k), torch.int32, dev, -77)]
    nws = max(moe.route_workspace_bytes(T, E, k), 16)
    ws_buf = torch.full((nws + 2 * GUARD,), 0x5A, dtype=torch.uint8, device=dev)
    # rows of the logits padded too: a stride of E + 3
    store = torch.full((T, E + 3), 60000.0, dtype=torch.float16, device=dev)
    store[:, :E] = torch.from_numpy(logits).to(dev)
    got = moe.route(store[:, :E], k, out=tuple(v for _, v in bufs) + (ws_buf[GUARD:GUARD + nws],))
    torch.cuda.synchronize()
    for (buf, _), fill, name in zip(bufs, (-77, -5.0, -77, -77, -77), ("expert_ids", "weights", "expert_offsets", "pair_token", "pair_pos")):
        _untouched(buf, fill, name)
    assert (ws_buf[:GUARD] == 0x5A).all() and (ws_buf[-GUARD:] == 0x5A).all(), "workspace: a guard element was written"
    return [t.cpu().numpy().copy() for t in got]


@pytest.mark.parametrize("name,logits,k", CASES, ids=[c[0] for c in CASES])
def test_route(moe, gpu, name, logits, k):
    """ids, offsets, pair_token and pair_pos equal the restatement; two launches are bit-equal; guards are untouched.  Weights: within
    `_moe_cases.route_weight_bound` of the float64 softmax - the bound is derived there from the op sequence: one rounding of the
    subtraction, the documented 1 ulp of expf (HIP math API documentation of ROCm, single-precision table; the figure is quoted: the
    device library ships as bitcode, without that page), k - 1 additions and the division."""
    want = K.route_ref(logits, k)
    got = _route(moe, logits, k, gpu)
    for i, what in ((0, "expert_ids"), (2, "expert_offsets"), (3, "pair_token"), (4, "pair_pos")):
        assert got[i].dtype == np.int32 and np.array_equal(got[i], want[i]), f"{name}: {what} differs"
    err = np.abs(got[1].astype(np.float64) - want[1])
    bound = K.route_weight_bound(logits, want[0], want[1])
    print(f"{name}: worst weight error {float((err / bound).max()):.3f} of the bound")
    assert (err <= bound).all(), f"{name}: weights beyond the bound, worst {float((err / bound).max()):.3f} of it"
    again = _route(moe, logits, k, gpu)
    for a, b in zip(got, again):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{name}: two launches differ"


def test_route_prefill_size(moe, gpu):
    """T k = 131 072 pairs (a long prompt): the multi-launch path over 128 chunks."""
    T, E, k = 65536, 8, 2
    logits = (np.random.default_rng(7).standard_normal((T, E)) * 2).astype(np.float16)
    want = K.route_ref(logits, k)
    got = [t.cpu().numpy() for t in moe.route(torch.from_numpy(logits).to(gpu), k)]
    for i in (0, 2, 3, 4):
        assert np.array_equal(got[i], want[i])
    assert (np.abs(got[1] - want[1]) <= K.route_weight_bound(logits, want[0], want[1])).all()


# ---- the grouped GEMMs --------------------------------------------------------------------------------------------------------------------
X_ROWS = 40
MODES = [("per_chn", 0), ("per_chn", 1), ("per_group", 0)]


def _problem(mode, E, N, Kk, seed):
    """E experts' weights (oracle.synth, one problem per expert) over ONE set of X_ROWS activation rows."""
    probs = [(synth.per_channel_problem if mode == "per_chn" else synth.per_group_problem)(X_ROWS, N, Kk, seed=seed + e) for e in range(E)]
    names = ("qweight", "wscales", "w_szs") if mode == "per_chn" else ("qweight", "wscales", "s2_scales", "s2_zeros")
    stacked = {n: np.stack([p[n] for p in probs]) for n in names}
    act = {n: probs[0][n] for n in (("A", "ascales", "a_ssums") if mode == "per_chn" else ("A", "ascales"))}
    return probs, stacked, act


def _lin(moe, mode, stacked, dev):
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)       # noqa: E731
    if mode == "per_chn":
        return moe.MoELinear.from_tensors(dict(qweight=d(stacked["qweight"]), s1_scales=d(stacked["wscales"]), s1_szeros=d(stacked["w_szs"])), -1)
    return moe.MoELinear.from_tensors(dict(qweight=d(stacked["qweight"]), s1_scales=d(stacked["wscales"]), s2_scales=d(stacked["s2_scales"]),
                                           s2_zeros=d(stacked["s2_zeros"])), 128)


@pytest.mark.parametrize("Kk", [128, 256, 384, 1024])
@pytest.mark.parametrize("mt", [1, 2, 4])
@pytest.mark.parametrize("mode,epi", MODES, ids=["per_chn-epi0", "per_chn-epi1", "per_group"])
def test_grouped_gemm(moe, gpu, mode, epi, mt, Kk):
    """For N in 64, 192, 512: rows per expert 0, 1, 15, 16, 17, 16 mt, 16 mt + 1 under the plan with `mt` m-tiles; row_src with repeats in
    a non-monotone order, and the same rows gathered with row_src = None; padded x and out strides; 0 ulp against the oracle of every
    pair's (expert, source row); bit-equal to the dense op per expert on the gathered rows; rows >= P and the guard columns untouched; the
    second launch equals the first.  K: one k-step (128), two, three for four waves (384: fewer steps than waves, a count the waves do
    not divide), eight."""
    import qserve_backend.qgemm_w4a8_per_chn as gemm_chn
    import qserve_backend.qgemm_w4a8_per_group as gemm_grp
    from qserve_amd._lib import check, lib
    counts = K.ROWS_PER_EXPERT[mt]
    E, P = len(counts), sum(counts)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    rng = np.random.default_rng(100 * mt + Kk)
    row_src = rng.integers(0, X_ROWS, size=P).astype(np.int32)            # repeats (P > X_ROWS), no order
    assert len(set(row_src.tolist())) < P and (np.diff(row_src) < 0).any()
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(gpu)       # noqa: E731
    check(lib.qs_set_gemm_epilogue(epi), "epilogue")
    try:
        for N in (64, 192, 512):
            plan = moe.gemm_plan(P, E, N, Kk)
            assert plan[0] == mt and plan[2] >= K.true_row_blocks(counts, mt)
            probs, stacked, act = _problem(mode, E, N, Kk, seed=7 * N + Kk)
            lin = _lin(moe, mode, stacked, gpu)
            # ---- the oracle, pair by pair
            want = np.zeros((P, N), np.float16)
            for e in range(E):
                rows = row_src[offsets[e]:offsets[e + 1]]
                if rows.size == 0:
                    continue
                if mode == "per_chn":
                    acc = w4a8.gemm_per_chn_acc(act["A"][rows], probs[e]["qweight"])
                    want[offsets[e]:offsets[e + 1]] = w4a8.epilogue_per_chn(acc, probs[e]["wscales"], act["ascales"][rows], probs[e]["w_szs"],
                                                                             act["a_ssums"][rows], fma=bool(epi))
                else:
                    want[offsets[e]:offsets[e + 1]] = w4a8.gemm_per_group(act["A"][rows], probs[e]["qweight"], probs[e]["s2_zeros"],
                                                                           probs[e]["s2_scales"], probs[e]["wscales"], act["ascales"][rows])[1]
            # ---- padded x / out, gathered through row_src
            x_store = torch.full((X_ROWS, Kk + 16), 99, dtype=torch.int8, device=gpu)
            x_store[:, :Kk] = d(act["A"])
            x = x_store[:, :Kk]
            scale, ssum = d(act["ascales"]), d(act["a_ssums"]) if mode == "per_chn" else None
            fill = float(np.float16(-1234.0))
            out_store = torch.full((P + 3, N + 8), fill, dtype=torch.float16, device=gpu)
            out = out_store[:P, :N]
            moe.grouped_gemm(x, scale, ssum, d(offsets), lin, out, row_src=d(row_src))
            torch.cuda.synchronize()
            first = out_store.cpu().numpy().copy()
            assert np.array_equal(first[:P, :N].view(np.uint16), want.view(np.uint16)), f"N={N}: not 0 ulp against the oracle"
            assert (first[P:] == fill).all() and (first[:, N:] == fill).all(), f"N={N}: a row >= P or a guard column was written"
            moe.grouped_gemm(x, scale, ssum, d(offsets), lin, out, row_src=d(row_src))
            torch.cuda.synchronize()
            assert np.array_equal(out_store.cpu().numpy().view(np.uint16), first.view(np.uint16)), f"N={N}: the second launch differs"
            # ---- row_src = None on the rows gathered beforehand
            gx = d(act["A"][row_src])
            gs, gsum = d(act["ascales"][row_src]), d(act["a_ssums"][row_src]) if mode == "per_chn" else None
            out2 = torch.full((P, N), fill, dtype=torch.float16, device=gpu)
            moe.grouped_gemm(gx, gs, gsum, d(offsets), lin, out2)
            assert np.array_equal(out2.cpu().numpy().view(np.uint16), want.view(np.uint16)), f"N={N}: row_src = None differs"
            # ---- the dense entry per expert on the gathered rows
            for e in range(E):
                lo, hi = int(offsets[e]), int(offsets[e + 1])
                if hi == lo:
                    continue
                dense = torch.empty((hi - lo, N), dtype=torch.float16, device=gpu)
                w = lin.expert(e)
                if mode == "per_chn":
                    gemm_chn.gemm_forward_cuda(gx[lo:hi].contiguous(), w["qweight"], w["s1_scales"], gs[lo:hi].contiguous(), w["s1_szeros"],
                                               gsum[lo:hi].contiguous(), dense)
                else:
                    gemm_grp.gemm_forward_cuda(gx[lo:hi].contiguous(), w["qweight"], w["s2_zeros"], w["s2_scales"], w["s1_scales"],
                                               gs[lo:hi].contiguous(), dense)
                assert torch.equal(dense.view(torch.int16), out[lo:hi].contiguous().view(torch.int16)), f"N={N}: expert {e} differs from the dense op"
    finally:
        check(lib.qs_set_gemm_epilogue(0), "epilogue")


# ---- combine ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [64, 256])
@pytest.mark.parametrize("T", [1, 130])
@pytest.mark.parametrize("k", [1, 2, 8])
def test_combine(moe, gpu, k, T, N):
    rng = np.random.default_rng(1000 * k + T + N)
    y = (rng.standard_normal((T * k, N)) * 3).astype(np.float16)
    w = rng.random((T, k)).astype(np.float32)
    w = (w / w.sum(axis=1, keepdims=True)).astype(np.float32)
    pair_pos = rng.permutation(T * k).astype(np.int32).reshape(T, k)
    want = K.combine_ref(y, w, pair_pos)
    fill = float(np.float16(-77.0))
    y_store = torch.zeros((T * k, N + 8), dtype=torch.float16, device=gpu)
    y_store[:, :N] = torch.from_numpy(y).to(gpu)
    out_store = torch.full((T + 2, N + 16), fill, dtype=torch.float16, device=gpu)
    moe.combine(out_store[:T, :N], y_store[:, :N], torch.from_numpy(w).to(gpu), torch.from_numpy(pair_pos).to(gpu))
    got = out_store.cpu().numpy()
    assert np.array_equal(got[:T, :N].view(np.uint16), want.view(np.uint16))
    assert (got[T:] == fill).all() and (got[:, N:] == fill).all()
