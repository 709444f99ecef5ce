"""GPU parity of the activation-side kernels (they define the GEMM's A / ascales / a_ssums)."""
import numpy as np
import pytest
import torch

from _helpers import dev, ulp_diff_f16
from oracle import fused

pytestmark = pytest.mark.gpu

# Measured deviations of the row statistics per shape -> gpurun_out/round6_row_stats.json (copied to profiles/): the
# thresholds asserted below are those measurements + margin (VERDICT r05 "weak" 3), not a-priori guesses.
_ROW_STATS = {}


def _record_row_stats(name, **entry):
    import json
    import os
    _ROW_STATS[name] = {k: (float(v) if isinstance(v, (float, np.floating)) else int(v)) for k, v in entry.items()}
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    try:
        os.makedirs(os.path.join(root, "gpurun_out"), exist_ok=True)
        with open(os.path.join(root, "gpurun_out", "round6_row_stats.json"), "w") as f:
            json.dump(dict(note="max deviation of the HIP row kernels' statistics from oracle/fused.py per (op, tokens, hidden): "
                                "fp16 ulps and absolute; `sum_vs_exact` = against the order-free exact sum, `sum_vs_reference_order` "
                                "= against the reference's half-accumulator order (what qs_set_row_sum_order(1) reproduces bit for bit)",
                           cases=_ROW_STATS), f, indent=1, sort_keys=True)
    except OSError:
        pass


def _f32(t):
    return t.cpu().numpy().astype(np.float32)


def _check_int8(q_gpu, q_ref, pre):
    """int8 must match exactly except where the pre-rounding fp32 value is within 2e-3 of a tie (the rounding then
    depends on fp32 summation order of the row statistics, which differs between any two implementations)."""
    q = q_gpu.cpu().numpy().astype(np.int32)
    frac = np.abs(pre - np.floor(pre) - 0.5)
    safe = frac > 2e-3
    assert np.array_equal(q[safe], q_ref.astype(np.int32)[safe])
    assert np.abs(q - q_ref.astype(np.int32)).max() <= 1


@pytest.mark.parametrize("T,H", [(1, 64), (5, 4096), (64, 4096), (3, 14336), (2, 8192)])
def test_invoke_quant_fuse_sum(gpu, T, H):
    import qserve_backend.fused_kernels as op
    x = (np.random.default_rng(T + H).standard_normal((T, H)) * 2).astype(np.float16)
    q_ref, s_ref, sum_ref, pre = fused.quant_per_token(x, with_sum=True)
    out = torch.empty((T, H), dtype=torch.int8, device=gpu)
    sc = torch.empty((T,), dtype=torch.float16, device=gpu)
    sm = torch.empty((T,), dtype=torch.float16, device=gpu)
    op.invoke_quant_fuse_sum(out, dev(x), sm, sc)
    assert np.array_equal(sc.cpu().numpy().view(np.uint16), s_ref.view(np.uint16))       # amax is order independent
    assert np.array_equal(out.cpu().numpy(), q_ref)                                        # so the int8 are exact
    # the row sum: fp32 in the reference too (fused_kernels.cu:104-122), so only the fp32 ASSOCIATION differs from the oracle's
    # exact sum: <= 1 fp16 ulp of the result, or - where the row cancels to a small sum - <= 4 fp32 ulps of sum |x|
    ulps = ulp_diff_f16(sm.cpu().numpy(), sum_ref)
    absd = np.abs(_f32(sm) - sum_ref.astype(np.float32))
    l1 = np.abs(x.astype(np.float32)).sum(axis=-1)
    _record_row_stats(f"invoke_quant_fuse_sum_T{T}_H{H}", sum_max_ulps=ulps.max(), sum_max_abs=absd.max(),
                      sum_max_abs_over_l1=(absd / l1).max())
    assert ((ulps <= 1) | (absd <= 4 * 2.0 ** -24 * l1)).all(), (ulps.max(), absd.max())
    # ... and against the oracle's statement of THIS library's association (oracle.fused.hip_order_row_sum): bit for bit
    sum_hip = fused.quant_per_token(x, with_sum=True, sum_order="hip")[2]
    assert np.array_equal(sm.cpu().numpy().view(np.uint16), sum_hip.view(np.uint16))
    out2 = torch.empty_like(out)
    sc2 = torch.empty_like(sc)
    op.invoke_quant(out2, dev(x), sc2)
    assert torch.equal(out2, out) and torch.equal(sc2, sc)


# |default-order a_ssum - reference-order a_ssum| per hidden size: measured on the MI355X (profiles/round6_row_stats.json) + margin;
# it is the reference order's own fp16 accumulation noise (round 5 allowed 0.25 + 2e-3 * H / 64 = 0.378 at H = 4096)
SUM_VS_REF_ORDER_ATOL = {64: 0.004, 4096: 0.10, 8192: 0.125}     # measured: 0 / 0.0625 / 0.0625


@pytest.mark.parametrize("T,H", [(1, 64), (4, 4096), (64, 4096), (2, 8192)])
def test_rms_norm_general_fuse_sum(gpu, T, H):
    import qserve_backend.layernorm_ops as op
    r = np.random.default_rng(T * 7 + H)
    x = (r.standard_normal((T, H)) * 1.5 + 0.3).astype(np.float16)
    g = r.uniform(0.5, 1.5, H).astype(np.float16)
    q_ref, s_ref, sum_ref, pre = fused.rms_norm_general(x, g, 1e-5, with_sum=True)
    out = torch.empty((T, H), dtype=torch.int8, device=gpu)
    sc = torch.empty((T,), dtype=torch.float16, device=gpu)
    sm = torch.empty((T,), dtype=torch.float16, device=gpu)
    op.rms_norm_general_fuse_sum(out, dev(x), dev(g), sm, sc, 1e-5, True)
    assert ulp_diff_f16(sc.cpu().numpy(), s_ref).max() <= 1
    _check_int8(out, q_ref, pre)
    # a_ssum in the library's DEFAULT order (fp32 chains): against the order-free exact sum of the same fp16 values it is an fp32
    # association (<= 1 fp16 ulp); against the reference's half-accumulator order it differs by THAT order's fp16 rounding noise
    # (the reference-order form itself is bit-exact: test_rms_norm_general_reference_order_sum below).  Measured -> round6_row_stats.
    sum_exact = fused.rms_norm_general(x, g, 1e-5, with_sum=True, sum_order="fp32")[2]
    u_e = ulp_diff_f16(sm.cpu().numpy(), sum_exact)
    d_r = np.abs(_f32(sm) - sum_ref.astype(np.float32))
    _record_row_stats(f"rms_norm_general_fuse_sum_T{T}_H{H}", scale_max_ulps=ulp_diff_f16(sc.cpu().numpy(), s_ref).max(),
                      sum_vs_exact_max_ulps=u_e.max(), sum_vs_exact_max_abs=np.abs(_f32(sm) - sum_exact.astype(np.float32)).max(),
                      sum_vs_reference_order_max_abs=d_r.max(),
                      sum_vs_reference_order_max_ulps=ulp_diff_f16(sm.cpu().numpy(), sum_ref).max())
    assert u_e.max() <= 1 or np.abs(_f32(sm) - sum_exact.astype(np.float32)).max() <= 2e-3, u_e.max()
    assert d_r.max() <= SUM_VS_REF_ORDER_ATOL[H], d_r.max()
    # the oracle with the library's own fp32 association of mean / variance / row sum (stats_order = sum_order = "hip"):
    # int8 row, scale and sum BIT-EQUAL, rounding ties included
    q_h, s_h, sum_h, _ = fused.rms_norm_general(x, g, 1e-5, with_sum=True, sum_order="hip", stats_order="hip")
    assert np.array_equal(out.cpu().numpy(), q_h), int((out.cpu().numpy() != q_h).sum())
    assert np.array_equal(sc.cpu().numpy().view(np.uint16), s_h.view(np.uint16))
    assert np.array_equal(sm.cpu().numpy().view(np.uint16), sum_h.view(np.uint16))
    out2 = torch.empty_like(out)
    sc2 = torch.empty_like(sc)
    op.rms_norm_general(out2, dev(x), dev(g), sc2, 1e-5, True)
    assert torch.equal(out2, out) and torch.equal(sc2, sc)


@pytest.mark.parametrize("T,H", [(1, 64), (3, 72), (2, 1000), (4, 4096), (64, 4096), (2, 8192), (3, 5120), (2, 14336), (5, 1032)])
def test_rms_norm_general_reference_order_sum(gpu, T, H):
    """qs_set_row_sum_order(1): `a_ssums` in the reference's own order - per-thread HALF accumulators over the min(H, 1024)-thread
    stride partition, fp32 warp butterflies (layernorm_kernels.cu:275-306, reduction_utils.cuh:25-30,68-85) - BIT-EQUAL to
    oracle.fused.rms_norm_general(sum_order="reference"), in the stand-alone op and the add + norm pair fusion (the K-slice planes
    form: tests/test_row_extremes_gpu.py); int8 rows and scales are the default order's, bit for bit (the switch touches nothing else)."""
    import qserve_backend.layernorm_ops as op
    from qserve_amd import fused as fz
    from qserve_amd._lib import lib
    r = np.random.default_rng(T * 11 + H)
    x = (r.standard_normal((T, H)) * 1.5 + 0.3).astype(np.float16)
    g = r.uniform(0.5, 1.5, H).astype(np.float16)
    d = (r.standard_normal((T, H)) * 0.5).astype(np.float16)
    # (mean / variance in the library's fp32 association, so that the normalised fp16 values the sum runs over are the kernel's
    #  own, bit for bit; with the order-free statistics 1 row in ~30 differs by one fp16 ulp - a normalised value one rounding
    #  apart -, measured in round 6's first GPU run)
    q_ref, s_ref, sum_ref, pre = fused.rms_norm_general(x, g, 1e-5, with_sum=True, sum_order="reference", stats_order="hip")
    sum_ref_exact_stats = fused.rms_norm_general(x, g, 1e-5, with_sum=True, sum_order="reference")[2]

    def run():
        out = torch.empty((T, H), dtype=torch.int8, device=gpu)
        sc = torch.empty((T,), dtype=torch.float16, device=gpu)
        sm = torch.empty((T,), dtype=torch.float16, device=gpu)
        op.rms_norm_general_fuse_sum(out, dev(x), dev(g), sm, sc, 1e-5, True)
        return out, sc, sm
    out0, sc0, sm0 = run()
    assert lib.qs_set_row_sum_order(2) == -1 and lib.qs_get_row_sum_order() == 0
    try:
        assert lib.qs_set_row_sum_order(1) == 0 and lib.qs_get_row_sum_order() == 1
        out1, sc1, sm1 = run()
        assert torch.equal(out1, out0) and torch.equal(sc1.view(torch.int16), sc0.view(torch.int16))
        assert np.array_equal(sm1.cpu().numpy().view(np.uint16), sum_ref.view(np.uint16)), \
            (sm1.cpu().numpy(), sum_ref, ulp_diff_f16(sm1.cpu().numpy(), sum_ref).max())
        assert np.array_equal(out1.cpu().numpy(), q_ref) and np.array_equal(sc1.cpu().numpy().view(np.uint16), s_ref.view(np.uint16))
        # VERDICT r05 item 2a's bar (<= 1 fp16 ulp of the oracle with order-free statistics); where a row cancels to a small
        # sum one ulp of a NORMALISED VALUE (a rounding of one element flipped by an fp32 statistic one ulp apart) is several
        # ulps of the sum: absolute bound there
        d_ex = np.abs(_f32(sm1) - sum_ref_exact_stats.astype(np.float32))
        assert ((ulp_diff_f16(sm1.cpu().numpy(), sum_ref_exact_stats) <= 1) | (d_ex <= 4e-3)).all(), d_ex.max()
        # the pair fusion follows the switch and stays bit-identical to add ; norm
        xs = (x.astype(np.float32) - d.astype(np.float32)).astype(np.float16)     # hidden before the add
        h = dev(xs)
        q2 = torch.empty((T, H), dtype=torch.int8, device=gpu)
        sc2 = torch.empty((T,), dtype=torch.float16, device=gpu)
        sm2 = torch.empty((T,), dtype=torch.float16, device=gpu)
        fz.add_residual_rms_norm_general(q2, h, dev(d), dev(g), sc2, 1e-5, sm2)
        hsum = h.cpu().numpy()
        q3, s3, sum3, _ = fused.rms_norm_general(hsum, g, 1e-5, with_sum=True, sum_order="reference", stats_order="hip")
        assert np.array_equal(sm2.cpu().numpy().view(np.uint16), sum3.view(np.uint16))
        assert np.array_equal(q2.cpu().numpy(), q3) and np.array_equal(sc2.cpu().numpy().view(np.uint16), s3.view(np.uint16))
    finally:
        lib.qs_set_row_sum_order(0)
    out2, sc2, sm2 = run()
    assert torch.equal(sm2.view(torch.int16), sm0.view(torch.int16)), "the default order must be back"


@pytest.mark.parametrize("H", [64, 4096, 8192, 14336])
def test_all_zero_activation_rows(gpu, H):
    """An all-zero activation row (fused_kernels.cu:104-130: amax = 0 -> scale = half(0 / 127) = 0, tmp_scale = 127 / 0 = inf,
    0 * inf = NaN -> cvt.rni.sat.s8 of NaN = 0): int8 row 0, scale 0, row sum 0 - and its neighbours in the batch are untouched.
    The general norm of a zero row: mean 0, variance 0, normalised values 0, amax = half(1e-6) (layernorm_kernels.cu:285),
    scale = half(1e-6 / 127) = 0 in fp16, row 0, sum 0."""
    import qserve_backend.fused_kernels as fk
    import qserve_backend.layernorm_ops as ln
    from qserve_amd import fused as fz
    r = np.random.default_rng(H)
    x = (r.standard_normal((5, H)) * 2).astype(np.float16)
    x[1] = 0
    x[4] = 0
    x[3, 1:] = 0                                          # one non-zero element: amax = |x[3, 0]|
    q_ref, s_ref, sum_ref, _ = fused.quant_per_token(x, with_sum=True)
    assert not q_ref[1].any() and s_ref[1] == 0 and sum_ref[1] == 0
    out = torch.full((5, H), 77, dtype=torch.int8, device=gpu)
    sc = torch.full((5,), 7.0, dtype=torch.float16, device=gpu)
    sm = torch.full((5,), 7.0, dtype=torch.float16, device=gpu)
    fk.invoke_quant_fuse_sum(out, dev(x), sm, sc)
    assert np.array_equal(out.cpu().numpy(), q_ref)
    assert np.array_equal(sc.cpu().numpy().view(np.uint16), s_ref.view(np.uint16))
    assert np.array_equal(sm.cpu().numpy()[[1, 4]].view(np.uint16), sum_ref[[1, 4]].view(np.uint16))
    assert ulp_diff_f16(sm.cpu().numpy(), sum_ref).max() <= 1
    out2 = torch.full_like(out, 55)
    sc2 = torch.full_like(sc, 5.0)
    fk.invoke_quant(out2, dev(x), sc2)
    assert torch.equal(out2, out) and torch.equal(sc2.view(torch.int16), sc.view(torch.int16))
    if H <= 8192:
        g = r.uniform(0.5, 1.5, H).astype(np.float16)
        q_ref, s_ref, sum_ref, pre = fused.rms_norm_general(x, g, 1e-5, with_sum=True, sum_order="fp32")
        assert not q_ref[1].any() and sum_ref[1] == 0
        ln.rms_norm_general_fuse_sum(out, dev(x), dev(g), sm, sc, 1e-5, True)
        assert np.array_equal(out.cpu().numpy()[[1, 4]], q_ref[[1, 4]])
        assert np.array_equal(sc.cpu().numpy()[[1, 4]].view(np.uint16), s_ref[[1, 4]].view(np.uint16))
        assert np.array_equal(sm.cpu().numpy()[[1, 4]].view(np.uint16), sum_ref[[1, 4]].view(np.uint16))
        _check_int8(out, q_ref, pre)
    # silu(0) * 0 = 0: the same degenerate row through the silu.mul + quant fusion
    y = (r.standard_normal((3, 2 * H)) * 2).astype(np.float16)
    y[1] = 0
    qq = torch.full((3, H), 9, dtype=torch.int8, device=gpu)
    ss = torch.full((3,), 9.0, dtype=torch.float16, device=gpu)
    mm = torch.full((3,), 9.0, dtype=torch.float16, device=gpu)
    fz.silu_and_mul_quant(qq, dev(y), ss, mm)
    assert not qq[1].any() and float(ss[1]) == 0 and float(mm[1]) == 0


def test_rms_norm_and_silu(gpu):
    import qserve_backend.activation_ops as act
    import qserve_backend.layernorm_ops as ln
    r = np.random.default_rng(8)
    x = r.standard_normal((9, 4096)).astype(np.float16)
    w = r.uniform(0.5, 1.5, 4096).astype(np.float16)
    out = torch.empty((9, 4096), dtype=torch.float16, device=gpu)
    ln.rms_norm(out, dev(x), dev(w), 1e-5)
    # half(x*rstd) can flip by one ulp with the fp32 summation order of the variance, the product by one more
    assert ulp_diff_f16(out.cpu().numpy(), fused.rms_norm(x, w, 1e-5)).max() <= 2
    y = (r.standard_normal((6, 2 * 14336)) * 2).astype(np.float16)
    o2 = torch.empty((6, 14336), dtype=torch.float16, device=gpu)
    act.silu_and_mul(o2, dev(y))
    # expf differs by an fp32 ulp between libraries: half(silu) can flip by one ulp, the product by one more
    assert ulp_diff_f16(o2.cpu().numpy(), fused.silu_and_mul(y)).max() <= 2


# ---- pair fusions (qserve_amd/fused.py): bit-identical to the two reference ops they replace -------------------------
@pytest.mark.parametrize("T,H", [(1, 64), (4, 4096), (64, 4096), (3, 8192), (2, 1000 * 8)])
@pytest.mark.parametrize("with_sum", [True, False])
def test_add_residual_norm_equals_op_pair(gpu, T, H, with_sum):
    import qserve_backend.layernorm_ops as ln
    from qserve_amd import fused as fz
    from qserve_amd.decode import residual_add_
    r = np.random.default_rng(T * 7 + H)
    h0 = dev((r.standard_normal((T, H)) * 3).astype(np.float16))
    d = dev((r.standard_normal((T, H)) * 2).astype(np.float16))
    w = dev(r.uniform(0.5, 1.5, H).astype(np.float16))

    def bufs():
        return (torch.empty((T, H), dtype=torch.int8, device=gpu), torch.full((T,), -1, dtype=torch.float16, device=gpu),
                torch.full((T,), -1, dtype=torch.float16, device=gpu))
    # reference sequence: torch-style add, then the norm op
    h_ref = h0.clone()
    q_ref, sc_ref, sm_ref = bufs()
    residual_add_(h_ref, d)
    assert torch.equal(h_ref, h0 + d)                      # the add itself is the plain fp16 add
    if with_sum:
        ln.rms_norm_general_fuse_sum(q_ref, h_ref, w, sm_ref, sc_ref, 1e-5, True)
    else:
        ln.rms_norm_general(q_ref, h_ref, w, sc_ref, 1e-5, True)
    h = h0.clone()
    q, sc, sm = bufs()
    fz.add_residual_rms_norm_general(q, h, d, w, sc, 1e-5, sm if with_sum else None)
    assert torch.equal(h, h_ref) and torch.equal(q, q_ref)
    assert torch.equal(sc.view(torch.int16), sc_ref.view(torch.int16))
    assert torch.equal(sm.view(torch.int16), sm_ref.view(torch.int16))


@pytest.mark.parametrize("T,D", [(1, 64), (5, 512), (64, 14336), (3, 24576 // 2), (2, 11008)])
@pytest.mark.parametrize("with_sum", [True, False])
def test_silu_mul_quant_equals_op_pair(gpu, T, D, with_sum):
    import qserve_backend.activation_ops as act
    import qserve_backend.fused_kernels as fk
    from qserve_amd import fused as fz
    x = dev((np.random.default_rng(T + D).standard_normal((T, 2 * D)) * 2).astype(np.float16))
    tmp = torch.empty((T, D), dtype=torch.float16, device=gpu)
    act.silu_and_mul(tmp, x)
    q_ref = torch.empty((T, D), dtype=torch.int8, device=gpu)
    sc_ref = torch.full((T,), -1, dtype=torch.float16, device=gpu)
    sm_ref = torch.full((T,), -1, dtype=torch.float16, device=gpu)
    if with_sum:
        fk.invoke_quant_fuse_sum(q_ref, tmp, sm_ref, sc_ref)
    else:
        fk.invoke_quant(q_ref, tmp, sc_ref)
    q, sc, sm = torch.empty_like(q_ref), torch.full_like(sc_ref, -1), torch.full_like(sm_ref, -1)
    fz.silu_and_mul_quant(q, x, sc, sm if with_sum else None)
    assert torch.equal(q, q_ref)
    assert torch.equal(sc.view(torch.int16), sc_ref.view(torch.int16))
    assert torch.equal(sm.view(torch.int16), sm_ref.view(torch.int16))


def test_decode_step_fused_pairs_equals_op_by_op(gpu):
    """Whole decode steps (tiny Llama, 2 layers, both weight granularities): fused-pair engine == op-by-op engine."""
    from qserve_amd.decode import TINY, DecodeEngine
    for gs in (-1, 128):
        outs = []
        for fuse in (False, True):
            eng = DecodeEngine(TINY, batch=5, prompt_len=70, max_new=4, group_size=gs, device="cuda:0", seed=3,
                               fuse_pairs=fuse)
            eng.prefill_cache(70)
            toks = []
            for _ in range(3):
                eng.step()
                toks.append(eng.tokens.clone())
            outs.append((eng.hidden.clone(), eng.final.clone(), torch.stack(toks)))
        for a, b in zip(outs[0], outs[1]):
            assert torch.equal(a, b)


def test_decode_step_with_k_slice_planes_equals_op_by_op(gpu):
    """The same at a width the K-slice planes form exists for (hidden 2048: down_proj leaves int32 planes, the next layer's add +
    norm + quant finishes it - qserve_amd/decode.py `proj_add_norm_quant`), planes for down and for down + o."""
    from qserve_amd.decode import TINY, DecodeEngine
    cfg = dict(TINY, hidden=2048, heads=16, kv_heads=4, inter=4096, layers=3)
    for gs in (-1, 128):
        outs = []
        for fuse, planes in ((False, ()), (True, ("down",)), (True, ("down", "o"))):
            eng = DecodeEngine(cfg, batch=5, prompt_len=70, max_new=4, group_size=gs, device="cuda:0", seed=3, fuse_pairs=fuse,
                               planes=planes)
            assert set(eng.planes) == set(planes)
            eng.prefill_cache(70)
            toks = []
            for _ in range(3):
                eng.step()
                toks.append(eng.tokens.clone())
            outs.append((eng.hidden.clone(), eng.final.clone(), torch.stack(toks)))
        for other in outs[1:]:
            for a, b in zip(outs[0], other):
                assert torch.equal(a, b)


def test_llama3_shape_steps_are_deterministic_and_equal_op_by_op(gpu):
    """The production geometry (Llama-3-8B widths, bs = 64, context 1033.., 4 layers): 48 hipGraph-replayed steps of the fused
    engine (pair fusions, K-slice planes, granule hand-over in the attention) give the same tokens on a second engine built
    from the same seed - the in-launch hand-offs cannot depend on timing -, and its first steps equal the op-by-op engine's bit for
    bit (tokens, residual stream, final norm)."""
    from qserve_amd.decode import LLAMA3_8B, DecodeEngine
    cfg = dict(LLAMA3_8B, layers=4)

    def make(fuse):
        e = DecodeEngine(cfg, batch=64, prompt_len=1024, max_new=64, device="cuda:0", seed=11, fuse_pairs=fuse)
        e.prefill_cache(1024 + 8)
        e.lengths.fill_(1033)
        return e
    runs = []
    for _ in range(2):
        e = make(True)
        assert "down" in e.planes
        e.capture()
        e.lengths.fill_(1033)
        toks = []
        for _ in range(48):
            e.run()
            toks.append(e.tokens.clone())
        torch.cuda.synchronize()
        runs.append((torch.stack(toks), e.hidden.clone()))
        del e
        torch.cuda.empty_cache()
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "fused steps are not reproducible"
    outs = []
    for fuse in (True, False):
        e = make(fuse)
        toks = []
        for _ in range(4):
            e.step()
            toks.append(e.tokens.clone())
        outs.append((torch.stack(toks), e.hidden.clone(), e.final.clone()))
        del e
        torch.cuda.empty_cache()
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_prefill_batched_equals_per_sequence(gpu):
    """Real prefill (norm+quant -> W4A8 GEMMs -> RoPE + quantised cache write -> causal flash attention -> ...) of a
    4-sequence batch equals the same sequences prefilled one by one, bit for bit: per-token ops, integer-exact GEMMs
    (different kernel families for different M) and per-sequence attention make the batch a pure concatenation."""
    from qserve_amd.decode import TINY, DecodeEngine
    P = 150
    toks = torch.randint(0, TINY["vocab"], (4 * P,), device=gpu, generator=torch.Generator(device=gpu).manual_seed(1))
    for gs in (-1, 128):
        big = DecodeEngine(TINY, batch=4, prompt_len=P, max_new=4, group_size=gs, device="cuda:0", seed=5)
        big.prefill(P, tokens=toks)
        for b in range(4):
            one = DecodeEngine(TINY, batch=1, prompt_len=P, max_new=4, group_size=gs, device="cuda:0", seed=5)
            one.prefill(P, tokens=toks[b * P:(b + 1) * P].contiguous())
            assert torch.equal(one.hidden[0], big.hidden[b])
            assert int(one.tokens[0]) == int(big.tokens[b])
        # and the cache it wrote is usable: decode steps run and stay finite
        for _ in range(3):
            big.step()
        assert torch.isfinite(big.hidden.float()).all()


@pytest.mark.parametrize("tp_world", [2, 4, 8])
def test_decode_engine_tp_rank_shapes_run(gpu, tp_world):
    """One rank's shard of the tensor-parallel Llama-3-8B step (2 layers; all-reduce is a no-op without a process
    group): every per-rank kernel shape the N>1 bench issues -- H/tp query heads over Hkv/tp KV heads, K-split o/down
    -- runs eagerly and under hipGraph capture, fused pairs == op-by-op, real prefill included."""
    from qserve_amd.decode import LLAMA3_8B, DecodeEngine
    cfg = dict(LLAMA3_8B, layers=2)
    outs = []
    for fuse in (False, True):
        eng = DecodeEngine(cfg, batch=8, prompt_len=96, max_new=8, device="cuda:0", seed=11, tp_rank=tp_world - 1,
                           tp_world=tp_world, fuse_pairs=fuse)
        eng.prefill(96)
        eng.step()
        eng.capture()
        eng.run()
        torch.cuda.synchronize()
        assert torch.isfinite(eng.hidden.float()).all()
        outs.append((eng.hidden.clone(), eng.tokens.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_piecewise_graphs_equal_eager_steps(gpu):
    """Tensor-parallel capture mode (one hipGraph per segment between the all-reduces) replays exactly the eager step
    sequence; so does the single-graph mode."""
    from qserve_amd.decode import LLAMA3_8B, DecodeEngine
    cfg = dict(LLAMA3_8B, layers=3)
    outs = []
    for mode in ("eager", "piecewise", "single"):
        eng = DecodeEngine(cfg, batch=4, prompt_len=80, max_new=12, device="cuda:0", seed=21, tp_rank=1, tp_world=4)
        eng.prefill_cache(80)
        if mode != "eager":
            got = eng.capture(piecewise=mode == "piecewise")   # executes ONE (warm-up) step; the capture pass only records
            if mode == "piecewise":
                assert eng.vocab_parallel and len(got) == 2 * 3 + 2   # 2 all-reduces per layer + the greedy head's exchange
        else:
            eng.step()
        for _ in range(3):
            eng.run()
        torch.cuda.synchronize()
        outs.append((eng.hidden.clone(), eng.tokens.clone(), eng.lengths.clone()))
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert torch.equal(a, b)


MODEL_SHAPES = {   # one layer of the reference's other supported dense models (qserve README model list)
    "llama2-13b": dict(hidden=5120, heads=40, kv_heads=40, inter=13824),
    "yi-34b": dict(hidden=7168, heads=56, kv_heads=8, inter=20480),
    "llama2-70b": dict(hidden=8192, heads=64, kv_heads=8, inter=28672),
    "qwen1.5-72b": dict(hidden=8192, heads=64, kv_heads=64, inter=24576),
    "mistral-7b": dict(hidden=4096, heads=32, kv_heads=8, inter=14336),
}


@pytest.mark.parametrize("name", sorted(MODEL_SHAPES))
@pytest.mark.parametrize("gs", [-1, 128])
def test_other_model_shapes_run_and_fuse_identically(gpu, name, gs):
    """Every kernel of the path at the layer shapes of the other dense models the reference lists (hidden sizes 5120 /
    7168 / 8192, GQA groups 1 / 7 / 8, K not a multiple of 1024): prefill + decode steps, eager and captured, fused
    pairs == op-by-op.  (Plumbing test.  The oracle comparisons for these shapes are per kernel - every GEMM of these
    layers in tests/test_gemm_gpu.py::test_other_model_shapes_exact, the GQA group sizes in tests/test_attention_gpu.py
    - and end to end, engine on the device against the engine on the oracle, in
    tests/test_loader.py::test_device_engine_matches_oracle_engine.)"""
    from qserve_amd.decode import DecodeEngine
    cfg = dict(MODEL_SHAPES[name], name=name, layers=1, vocab=1024, rope_theta=1e4, eps=1e-5)
    outs = []
    for fuse in (False, True):
        eng = DecodeEngine(cfg, batch=6, prompt_len=70, max_new=8, group_size=gs, device="cuda:0", seed=9, fuse_pairs=fuse)
        eng.prefill(70)
        eng.step()
        eng.capture()
        eng.run()
        torch.cuda.synchronize()
        assert torch.isfinite(eng.hidden.float()).all()
        outs.append((eng.hidden.clone(), eng.tokens.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_wave_reductions_round_like_the_shuffle_butterfly(gpu):
    """common.h wave_sum / wave_max (permlane swaps + DPP) == the __shfl_xor butterfly, bit for bit, in every lane: the
    row kernels' statistics (and with them every int8 activation byte) depend on that summation order."""
    import ctypes
    from qserve_amd._lib import check, lib
    g = torch.Generator(device=gpu).manual_seed(0)
    n = 64 * 4096
    x = (torch.randn((n,), device=gpu, generator=g) * torch.exp(torch.randn((n,), device=gpu, generator=g) * 3)).float()
    out = torch.zeros((n // 64, 4), device=gpu)
    check(lib.qs_debug_wave_reduce_selftest(x.data_ptr(), out.data_ptr(), n, torch.cuda.current_stream().cuda_stream), "selftest")
    torch.cuda.synchronize()
    o = out.view(torch.int32)
    assert torch.equal(o[:, 0], o[:, 1]), "wave_sum differs from the shuffle butterfly"
    assert torch.equal(o[:, 2], o[:, 3]), "wave_max differs from the shuffle butterfly"
    assert torch.allclose(out[:, 0], x.view(-1, 64).double().sum(1).float(), rtol=1e-4, atol=1e-3)
    assert torch.equal(out[:, 2], x.view(-1, 64).max(1).values)


# ---- greedy sampling helper ------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("rows,n,pad", [(1, 8, 0), (3, 1000, 0), (64, 128256, 0), (5, 152064, 0), (7, 4099, 5), (2, 300000, 0)])
def test_argmax_rows_is_first_maximum(gpu, rows, n, pad):
    """qs_argmax_rows against numpy's argmax (first maximum), incl. ties, a strided view, n % 8 != 0 and vocabularies
    larger than one pass."""
    from qserve_amd.decode import argmax_rows_
    r = np.random.default_rng(rows * 31 + n)
    stride = (n + pad + 7) // 8 * 8
    x = (r.standard_normal((rows, stride)) * 4).astype(np.float16)
    x[:, n:] = 100.0                                        # beyond the row: must never win
    if n >= 8:
        x[0, [n - 1, n // 2, 3]] = 50.0                      # ties: the first one counts
    xd = dev(x)
    want = np.argmax(x[:, :n].astype(np.float32), axis=1)
    from qserve_amd import _lib
    try:
        for split in (-1, 1, 2, 3, 8):                      # heuristic / one workgroup per row / rows split over workgroups
            _lib.lib.qs_debug_argmax_split(split)
            for rep in range(3):                            # the split form's keys and tickets reset themselves
                out = torch.full((rows,), -7, dtype=torch.int64, device=gpu)
                argmax_rows_(xd[:, :n], out)
                torch.cuda.synchronize()
                assert np.array_equal(out.cpu().numpy(), want), (split, rep)
        _lib.lib.qs_debug_argmax_split(4)
        out = torch.full((rows,), -7, dtype=torch.int64, device=gpu)
        s_ = torch.cuda.Stream()
        s_.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s_):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s_):
                argmax_rows_(xd[:, :n], out)
        for rep in range(3):
            out.fill_(-7)
            g.replay()
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy(), want), ("graph", rep)
    finally:
        _lib.lib.qs_debug_argmax_split(-1)
