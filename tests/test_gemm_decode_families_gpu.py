"""GPU parity of the two older W4A8 decode kernels at EVERY geometry they are built for, and of the W8A8 kernel at its edges.

`w4a8_gemm_splitk` (csrc/gemm_w4a8.hip) and `w4a8_gemm_pair` (csrc/gemm_w4a8_lds.hip) still serve real shapes (short K at a
decode batch, shapes no ring geometry fits, narrow tensor-parallel prefill shards), but the dispatcher's own choice reaches
only a few of their instantiations at oracle-sized shapes.  The rows of tests/_gemm_family_cases.py force each one by selection
code; tests/test_gemm_family_cases_cpu.py holds the planner to the geometry a row claims.  Reference: the CPU oracle
(oracle.w4a8) on oracle.synth problems, inside and outside the protective range.  Bar: int32 accumulators equal, fp16 output
0 ulp - no tolerance anywhere."""
import functools

import numpy as np
import pytest
import torch

import _gemm_family_cases as cases
from _helpers import dev, ulp_diff_f16
from oracle import synth, w4a8

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _problem(mode, M, N, K):
    """One problem per (mode, shape), shared by every row that uses it: (kernel operands, fp16-epilogue operands, the oracle's
    int32 accumulators, its fp16 output).  Nothing writes to any of it."""
    if mode == "per_channel":
        pr = synth.per_channel_problem(M, N, K, seed=M + N + K)
        acc, out = w4a8.gemm_per_chn(pr["A"], pr["qweight"], pr["wscales"], pr["ascales"], pr["w_szs"], pr["a_ssums"])
        return ([dev(pr[k]) for k in ("A", "qweight")],
                [dev(pr[k]) for k in ("wscales", "ascales", "w_szs", "a_ssums")], acc, out)
    pr = synth.per_group_problem(M, N, K, seed=M * 3 + N + K, valid=mode == "per_group")
    acc, out = w4a8.gemm_per_group(pr["A"], pr["qweight"], pr["s2_zeros"], pr["s2_scales"], pr["wscales"], pr["ascales"])
    return ([dev(pr[k]) for k in ("A", "qweight", "s2_zeros", "s2_scales")], [dev(pr[k]) for k in ("wscales", "ascales")], acc, out)


def _run_exact(gpu, code, mode, M, N, K):
    """Both output kinds of one GEMM under a selection code, each launched twice in a row into the first M rows of an
    (M + 2)-row buffer: exact against the oracle, the two launches bit-equal (nothing the first one leaves behind - arrival
    counters, LDS, slabs - changes the second), the guard rows untouched."""
    import qserve_backend.qgemm_w4a8_per_chn as opc
    import qserve_backend.qgemm_w4a8_per_group as opg
    from qserve_amd import _lib
    op = opc if mode == "per_channel" else opg
    operands, scales, acc_ref, out_ref = _problem(mode, M, N, K)
    accs = [torch.full((M + 2, N), -7, dtype=torch.int32, device=gpu) for _ in range(2)]
    outs = [torch.full((M + 2, N), float("nan"), dtype=torch.float16, device=gpu) for _ in range(2)]
    _lib.lib.qs_set_gemm_variant(code)
    try:
        for acc in accs:
            op.gemm_forward_acc(*operands, acc[:M])
        for out in outs:
            op.gemm_forward_cuda(*operands, *scales, out[:M])
    finally:
        _lib.lib.qs_set_gemm_variant(-1)
    accs = [a.cpu().numpy() for a in accs]
    outs = [o.cpu().numpy() for o in outs]
    assert np.array_equal(accs[0][:M], acc_ref), "int32 accumulators"
    assert ulp_diff_f16(outs[0][:M], out_ref).max() == 0, "fp16 output"
    assert np.array_equal(accs[1], accs[0]) and np.array_equal(outs[1].view(np.uint16), outs[0].view(np.uint16)), \
        "the second launch differs from the first"
    assert (accs[0][M:] == -7).all() and np.isnan(outs[0][M:]).all(), "rows beyond M were written"


def _ring_exact(gpu, code, M, N, K):
    """One forced ring GEMM (per-channel accumulators) against the oracle."""
    import qserve_backend.qgemm_w4a8_per_chn as opc
    from qserve_amd import _lib
    operands, _, acc_ref, _ = _problem("per_channel", M, N, K)
    acc = torch.full((M, N), -7, dtype=torch.int32, device=gpu)
    _lib.lib.qs_set_gemm_variant(code)
    try:
        opc.gemm_forward_acc(*operands, acc)
    finally:
        _lib.lib.qs_set_gemm_variant(-1)
    assert np.array_equal(acc.cpu().numpy(), acc_ref), f"ring {code}"


@pytest.fixture(scope="module")
def splitk_workspace(gpu):
    """A forced K-sliced ring launch refuses to run without the split-K workspace - once it has run, the workspace of this
    stream exists and a split-K launch with S > 1 really runs S blocks (without it the launcher falls back to S = 1)."""
    _ring_exact(gpu, 4221, 23, 64, 2048)


def _splitk_id(row):
    return "{}-M{}-N{}-K{}".format(cases.splitk_code(*row[:3]), *row[3:6])


@pytest.mark.parametrize("row", cases.SPLITK, ids=_splitk_id)
@pytest.mark.parametrize("mode", cases.MODES)
def test_split_k_geometry_vs_oracle(gpu, splitk_workspace, row, mode):
    mo, S, NW, M, N, K, _ = row
    _run_exact(gpu, cases.splitk_code(mo, S, NW), mode, M, N, K)


@pytest.mark.parametrize("M,N,K", cases.PAIR)
@pytest.mark.parametrize("mode", cases.MODES)
def test_pair_kernel_vs_oracle(gpu, M, N, K, mode):
    _run_exact(gpu, cases.PAIR_FORCED, mode, M, N, K)


@pytest.mark.parametrize("M,N,K", cases.PAIR_PREFILL)
@pytest.mark.parametrize("mode", ["per_channel", "per_group"])
def test_pair_kernel_prefill_route(gpu, M, N, K, mode):
    """The dispatcher's own choice: narrow tensor-parallel shards at more than 1024 tokens (18 token blocks of 64)."""
    _run_exact(gpu, -1, mode, M, N, K)


def test_split_k_and_ring_seam_share_the_arrival_counters(gpu, splitk_workspace):
    """Cross-block split-K and the K-sliced ring seam take their tickets from the same counters of the stream's workspace,
    each resetting what it used: alternating launches stay exact, neither leaves a ticket behind for the other."""
    _ring_exact(gpu, 4221, 23, 64, 2048)
    _run_exact(gpu, cases.splitk_code(2, 3, 2), "per_channel", 33, 192, 640)
    _ring_exact(gpu, 4422, 32, 256, 2048)
    _run_exact(gpu, cases.splitk_code(1, 2, 4), "per_group", 33, 192, 640)
    _ring_exact(gpu, 4221, 23, 64, 2048)


# the fmaf epilogue (qs_set_gemm_epilogue(1)) where test_gemm_gpu.py::test_epilogue_fma_convention_selectable does not reach:
# the pair kernel below 4 m-tiles and the split-K block that arrives last and finishes for the others
@pytest.mark.parametrize("code,M,N,K", [row[:4] for row in cases.EPILOGUE_FMA], ids=["pair-2-m-tiles", "split-k-last-arriver"])
def test_epilogue_fma_convention_in_the_old_decode_kernels(gpu, splitk_workspace, code, M, N, K):
    import qserve_backend.qgemm_w4a8_per_chn as op
    from qserve_amd import _lib
    lib = _lib.lib
    pr = synth.per_channel_problem(M, N, K, seed=M + N + K)
    acc = w4a8.gemm_per_chn_acc(pr["A"], pr["qweight"])
    scales = [pr[k] for k in ("wscales", "ascales", "w_szs", "a_ssums")]
    want = {0: w4a8.epilogue_per_chn(acc, *scales), 1: w4a8.epilogue_per_chn(acc, *scales, fma=True)}
    assert (want[0].view(np.uint16) != want[1].view(np.uint16)).any(), "the two conventions agree everywhere on this problem"
    args = [dev(pr[k]) for k in ("A", "qweight")] + [dev(s) for s in scales]
    try:
        lib.qs_set_gemm_variant(code)
        for conv in (1, 0, 1):
            assert lib.qs_set_gemm_epilogue(conv) == 0
            out = torch.full((M, N), float("nan"), dtype=torch.float16, device=gpu)
            op.gemm_forward_cuda(*args, out)
            assert np.array_equal(out.cpu().numpy().view(np.uint16), want[conv].view(np.uint16)), conv
    finally:
        lib.qs_set_gemm_epilogue(0)
        lib.qs_set_gemm_variant(-1)


@pytest.mark.parametrize("M,N,K", cases.W8A8)
def test_w8a8_vs_oracle(gpu, M, N, K):
    """The whole int8 range, -128 included, on both operands; waves of the last workgroup beyond N return without a store."""
    import qserve_backend.qgemm_w8a8 as op
    r = np.random.default_rng(M + N + K)
    A = r.integers(-128, 128, (M, K), dtype=np.int8)
    W = r.integers(-128, 128, (N, K), dtype=np.int8)
    A[M // 2, ::7] = -128
    W[N - 1, ::5] = -128            # meets A's -128 at every 35th k
    ws = r.uniform(0.002, 0.02, N).astype(np.float16)
    sa = r.uniform(0.005, 0.05, M).astype(np.float16)
    _, ref = w4a8.gemm_w8a8(A, W, ws, sa)
    out = torch.full((M + 2, N), float("nan"), dtype=torch.float16, device=gpu)
    op.w8a8_gemm_forward_cuda(dev(A), dev(W), dev(ws), dev(sa), out[:M])
    o = out.cpu().numpy()
    assert ulp_diff_f16(o[:M], ref).max() == 0
    assert np.isnan(o[M:]).all(), "rows beyond M were written"


@pytest.mark.parametrize("N,K", [(40, 64), (48, 96)], ids=["N-not-16", "K-not-64"])
def test_w8a8_refused_shapes_raise(gpu, N, K):
    import qserve_backend.qgemm_w8a8 as op
    A = torch.zeros((4, K), dtype=torch.int8, device=gpu)
    W = torch.zeros((N, K), dtype=torch.int8, device=gpu)
    ws = torch.ones((N,), dtype=torch.float16, device=gpu)
    sa = torch.ones((4,), dtype=torch.float16, device=gpu)
    out = torch.empty((4, N), dtype=torch.float16, device=gpu)
    with pytest.raises(RuntimeError):
        op.w8a8_gemm_forward_cuda(A, W, ws, sa, out)
