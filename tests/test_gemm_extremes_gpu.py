"""Every W4A8 / W8A8 GEMM family on the extreme, structured operands of tests/_gemm_extreme_cases.py: accumulators of 2^24 and
beyond that fp32 cannot hold, A = -128 and weight bytes of -128, K slices that are large and cancel, a_ssums = +-inf and 0 * inf in the
per-channel epilogue.  The random problems of the other GEMM tests stay three orders of magnitude below 2^24, where integer and fp32
combination of K slices, and a truncating and a rounding conversion, cannot be told apart; here they can.

Reference: oracle.w4a8 on the CPU (tests/test_gemm_extremes_cpu.py holds it to the int64 matmul on these operands, and every row to the
plan it names).  No tolerance anywhere: int32 accumulators equal; fp16 outputs bit for bit wherever the oracle is not NaN, and NaN
exactly where it is; per-channel under both epilogue conventions; rows beyond M, guard columns and sentinels untouched; a second launch
equal to the first."""
import numpy as np
import pytest
import torch

import _gemm_extreme_cases as cases
from _helpers import dev, ulp_diff_f16

pytestmark = pytest.mark.gpu
FILL = float(np.float16(-1234.0))                       # fp16 guard value: NaN is a legitimate output here


def _rows(*families):
    rows = [r for r in cases.TABLE if r.family in families]
    return pytest.mark.parametrize("row", rows, ids=[cases.row_id(r) for r in rows])


def _same_f16(got, want, what):
    """Bit for bit wherever `want` is not NaN; NaN exactly where `want` is."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN at other places"
    assert np.array_equal(got.view(np.uint16)[~nan], want.view(np.uint16)[~nan]), f"{what}: fp16 bits differ"


def _operands(pr):
    """(kernel operands, fp16-epilogue operands) on the device."""
    if pr["mode"] == "per_channel":
        return [dev(pr[k]) for k in ("A", "qweight")], [dev(pr[k]) for k in ("wscales", "ascales", "w_szs", "a_ssums")]
    return [dev(pr[k]) for k in ("A", "qweight", "s2_zeros", "s2_scales")], [dev(pr[k]) for k in ("wscales", "ascales")]


def _ops(pr):
    import qserve_backend.qgemm_w4a8_per_chn as opc
    import qserve_backend.qgemm_w4a8_per_group as opg
    return opc if pr["mode"] == "per_channel" else opg


def _oracle(row):
    """(problem, exact int32 accumulators, {convention: fp16 output}) of a row."""
    pr = cases.row_problem(row)
    acc = cases.oracle_acc(pr)
    convs = (0, 1) if row.mode == "per_channel" else (0,)
    return pr, acc, {c: cases.oracle_out(pr, acc, fma=bool(c)) for c in convs}


def _run_dense(gpu, row, select):
    """Both output kinds under the selections `select` (lists of codes set in order before the launches), each launched twice into the
    first M rows of an (M + 2)-row buffer."""
    from qserve_amd import _lib
    lib = _lib.lib
    pr, acc_ref, out_ref = _oracle(row)
    assert np.array_equal(acc_ref.astype(np.int64), cases.problem_acc(*cases.row_problem_key(row)))
    op, (operands, scales), M, N = _ops(pr), _operands(pr), row.M, row.N
    try:
        for codes in select:
            for code in codes:
                lib.qs_set_gemm_variant(code)
            accs = [torch.full((M + 2, N), -7, dtype=torch.int32, device=gpu) for _ in range(2)]
            for acc in accs:
                op.gemm_forward_acc(*operands, acc[:M])
            accs = [a.cpu().numpy() for a in accs]
            assert np.array_equal(accs[0][:M], acc_ref), f"{codes}: int32 accumulators differ from the integer matmul"
            assert np.array_equal(accs[1], accs[0]), f"{codes}: the second launch differs from the first"
            assert (accs[0][M:] == -7).all(), f"{codes}: rows beyond M were written"
            for conv, want in out_ref.items():
                assert lib.qs_set_gemm_epilogue(conv) == 0
                outs = [torch.full((M + 2, N), FILL, dtype=torch.float16, device=gpu) for _ in range(2)]
                for out in outs:
                    op.gemm_forward_cuda(*operands, *scales, out[:M])
                outs = [o.cpu().numpy() for o in outs]
                _same_f16(outs[0][:M], want, f"{codes}, epilogue {conv}")
                assert np.array_equal(outs[1].view(np.uint16), outs[0].view(np.uint16)), f"{codes}: the second launch differs from the first"
                assert (outs[0][M:] == FILL).all(), f"{codes}: rows beyond M were written"
    finally:
        lib.qs_set_gemm_epilogue(0)
        lib.qs_set_gemm_variant(5000)
        lib.qs_set_gemm_variant(3200)
        lib.qs_set_gemm_variant(-1)


@pytest.fixture(scope="module")
def splitk_workspace(gpu):
    """A forced K-sliced ring launch creates the split-K workspace of this stream; without it a cross-block split-K launch falls back
    to S = 1 (tests/test_gemm_decode_families_gpu.py)."""
    import qserve_backend.qgemm_w4a8_per_chn as opc
    from qserve_amd import _lib
    pr = cases.problem("per_channel", 17, 64, 2048, "q15")
    acc = torch.full((17, 64), -7, dtype=torch.int32, device=gpu)
    _lib.lib.qs_set_gemm_variant(4221)
    try:
        opc.gemm_forward_acc(dev(pr["A"]), dev(pr["qweight"]), acc)
    finally:
        _lib.lib.qs_set_gemm_variant(-1)
    assert np.array_equal(acc.cpu().numpy(), cases.oracle_acc(pr))


@_rows("own", "pair")
def test_planners_choice_and_pair_kernel(gpu, row):
    _run_dense(gpu, row, [[row.code]])


@_rows("splitk")
def test_split_k_geometries(gpu, splitk_workspace, row):
    _run_dense(gpu, row, [[row.code]])


@_rows("tiled", "wide")
def test_tiled_and_wide_kernels(gpu, row):
    """Three workgroups walking the tiles (3220) and one workgroup per tile (3210)."""
    _run_dense(gpu, row, [[row.code, 3220], [row.code, 3210]])


@_rows("ring")
def test_ring_geometries(gpu, row):
    """K-sliced geometries with the slices across the XCDs and on one XCD (ring flag 4096)."""
    sliced = cases.ring_geometry(row.code)[2] > 1
    _run_dense(gpu, row, [[5000, row.code], [5000 + 4096, row.code]] if sliced else [[row.code]])


@_rows("planes")
def test_planes_finished_by_the_row_kernel(gpu, row):
    """The planes sum to the exact accumulators, and add_residual_rms_norm_general_planes on them leaves the bits of the dense GEMM
    followed by add_residual_rms_norm_general - residual stream, int8 row, scale, row sum - under both epilogue conventions."""
    from qserve_amd import _lib, fused
    lib = _lib.lib
    pr, acc_ref, out_ref = _oracle(row)
    op, (operands, scales), M, N, K = _ops(pr), _operands(pr), row.M, row.N, row.K
    per_group = row.mode != "per_channel"
    g = torch.Generator(device=gpu).manual_seed(M + N)
    hidden = (torch.randn((M, N), device=gpu, generator=g) * 0.7).half()
    gamma = (torch.rand((N,), device=gpu, generator=g) + 0.5).half()
    try:
        lib.qs_set_gemm_variant(row.code)
        fused._PLANES_PLAN["nocache"] = True
        ks = fused.gemm_planes_plan(M, N, K, per_group)
        assert ks == row.plan[0]
        both = [torch.full((ks, M, N), 12345, dtype=torch.int32, device=gpu) for _ in range(2)]
        for planes in both:
            fused.gemm_planes(*operands[:2], planes, *operands[2:])
    finally:
        lib.qs_set_gemm_variant(-1)
        fused._PLANES_PLAN.clear()
    planes = both[0]
    assert torch.equal(both[0], both[1]), "the second launch differs from the first"
    assert np.array_equal(planes.sum(dim=0, dtype=torch.int64).cpu().numpy(), acc_ref.astype(np.int64)), "planes do not sum to the accumulators"
    try:
        for conv, want in out_ref.items():
            assert lib.qs_set_gemm_epilogue(conv) == 0
            delta = torch.full((M, N), FILL, dtype=torch.float16, device=gpu)
            op.gemm_forward_cuda(*operands, *scales, delta)
            _same_f16(delta.cpu().numpy(), want, f"dense GEMM, epilogue {conv}")
            res = []
            for from_planes in (False, True):
                h = hidden.clone()
                q = torch.full((M + 1, N), 77, dtype=torch.int8, device=gpu)
                sc = scales[1].clone() if from_planes else torch.empty((M,), dtype=torch.float16, device=gpu)
                sm = None if per_group else (scales[3].clone() if from_planes else torch.full((M,), 3.0, dtype=torch.float16, device=gpu))
                if not from_planes:
                    fused.add_residual_rms_norm_general(q[:M], h, delta, gamma, sc, 1e-5, sm)
                elif per_group:
                    fused.add_residual_rms_norm_general_planes(q[:M], h, planes, scales[0], sc, gamma, sc, 1e-5)
                else:       # the GEMM's activation scale / sum live where the row kernel writes its own (as in the decode engine)
                    fused.add_residual_rms_norm_general_planes(q[:M], h, planes, scales[0], sc, gamma, sc, 1e-5, w_szs=scales[2], a_ssums=sm,
                                                               input_sum=sm)
                assert (q[M:] == 77).all(), "rows beyond M were written"
                res.append((h.cpu().numpy(), q[:M].cpu().numpy(), sc.cpu().numpy(), None if sm is None else sm.cpu().numpy()))
            (h1, q1, sc1, sm1), (h2, q2, sc2, sm2) = res
            _same_f16(h2, h1, f"epilogue {conv}: residual stream")
            _same_f16(sc2, sc1, f"epilogue {conv}: scale")
            if sm1 is not None:
                _same_f16(sm2, sm1, f"epilogue {conv}: row sum")
            assert np.array_equal(q2, q1), f"epilogue {conv}: int8 row differs"
    finally:
        lib.qs_set_gemm_epilogue(0)


@_rows("gate_up")
def test_gate_up_silu_mul(gpu, row):
    """One call == the plain GEMM entry followed by activation_ops.silu_and_mul, bit for bit (as one launch where the kernel has the
    activation epilogue, as two launches, and without scratch); against the oracle within the two fp16 ulps the exponential's library
    leaves (tests/test_gemm_gpu.py::test_gate_up_silu_mul_vs_oracle_and_op_pair), where the oracle's GEMM output is finite."""
    import qserve_backend.activation_ops as act
    from oracle import fused as ofused
    from qserve_amd import _lib, fused as fz
    lib = _lib.lib
    pr, _, out_ref = _oracle(row)
    op, (operands, scales), M, N = _ops(pr), _operands(pr), row.M, row.N
    fusedop = fz.gemm_silu_and_mul_per_chn if row.mode == "per_channel" else fz.gemm_silu_and_mul_per_group
    one_launch_only = not (4200 <= row.code < 4500) and row.plan[0] != cases.F_SPLITK     # (else the call needs its scratch)
    try:
        for conv, y_ref in out_ref.items():
            assert lib.qs_set_gemm_epilogue(conv) == 0
            y = torch.full((M, N), FILL, dtype=torch.float16, device=gpu)
            pair = torch.empty((M, N // 2), dtype=torch.float16, device=gpu)
            op.gemm_forward_cuda(*operands, *scales, y)
            _same_f16(y.cpu().numpy(), y_ref, f"plain GEMM, epilogue {conv}")
            act.silu_and_mul(pair, y)
            want = pair.cpu().numpy()
            lib.qs_set_gemm_variant(row.code)
            outs = []
            for two_launches in (0, 1):
                lib.qs_set_gemm_variant(3300 + two_launches)
                for _ in range(2):
                    out = torch.full((M + 1, N // 2), FILL, dtype=torch.float16, device=gpu)
                    tmp = torch.empty((M, N), dtype=torch.float16, device=gpu)
                    fusedop(*operands, *scales, out[:M], tmp)
                    assert (out[M:] == FILL).all(), "rows beyond M were written"
                    outs.append(out[:M].cpu().numpy())
            if one_launch_only:
                lib.qs_set_gemm_variant(3300)
                out = torch.full((M, N // 2), FILL, dtype=torch.float16, device=gpu)
                fusedop(*operands, *scales, out, None)
                outs.append(out.cpu().numpy())
            lib.qs_set_gemm_variant(3300)
            lib.qs_set_gemm_variant(-1)
            for o in outs:
                _same_f16(o, want, f"epilogue {conv}: one call against the op pair")
            with np.errstate(over="ignore", invalid="ignore"):
                ref = ofused.silu_and_mul(y_ref)
            ok = np.isfinite(y_ref[:, :N // 2].astype(np.float32)) & np.isfinite(y_ref[:, N // 2:].astype(np.float32))
            assert ok.any() and not np.isnan(ref[ok]).any() and not np.isnan(want[ok]).any()
            assert ulp_diff_f16(want[ok], ref[ok]).max() <= 2
    finally:
        lib.qs_set_gemm_epilogue(0)
        lib.qs_set_gemm_variant(3300)
        lib.qs_set_gemm_variant(-1)


@_rows("moe")
def test_grouped_gemm(gpu, row):
    """Two experts - the row's weights and all-zero nibbles - over 14 source rows, every pattern twice, row_src with repeats, padded x and out:
    bit-equal to the oracle of every pair's (expert, source row), to the dense entry per expert on the gathered rows, rows >= P and the
    guard columns untouched, the second launch equal to the first."""
    from qserve_amd import _lib, moe
    lib = _lib.lib
    pr = cases.row_problem(row)
    experts = [pr, cases.moe_zero_expert(pr)]
    offsets, row_src = cases.moe_routing(row)
    P, N, K, per_chn = row.M, row.N, row.K, row.mode == "per_channel"
    assert moe.gemm_plan(P, 2, N, K) == row.plan
    names = ("qweight", "wscales", "w_szs") if per_chn else ("qweight", "wscales", "s2_scales", "s2_zeros")
    stacked = {n: dev(np.stack([e[n] for e in experts])) for n in names}
    if per_chn:
        lin = moe.MoELinear.from_tensors(dict(qweight=stacked["qweight"], s1_scales=stacked["wscales"], s1_szeros=stacked["w_szs"]), -1)
    else:
        lin = moe.MoELinear.from_tensors(dict(qweight=stacked["qweight"], s1_scales=stacked["wscales"], s2_scales=stacked["s2_scales"],
                                              s2_zeros=stacked["s2_zeros"]), 128)
    op = _ops(pr)
    x_store = torch.full((cases.MOE_X_ROWS, K + 16), 99, dtype=torch.int8, device=gpu)
    x_store[:, :K] = dev(pr["A"])
    x, scale, ssum = x_store[:, :K], dev(pr["ascales"]), dev(pr["a_ssums"]) if per_chn else None
    try:
        for conv in (0, 1) if per_chn else (0,):
            assert lib.qs_set_gemm_epilogue(conv) == 0
            want = np.zeros((P, N), np.float16)
            for e, ex in enumerate(experts):
                rows = row_src[offsets[e]:offsets[e + 1]]
                sub = dict(ex, A=pr["A"][rows], ascales=pr["ascales"][rows])
                if per_chn:
                    sub["a_ssums"] = pr["a_ssums"][rows]
                want[offsets[e]:offsets[e + 1]] = cases.oracle_out(sub, cases.oracle_acc(sub), fma=bool(conv))
            out_store = torch.full((P + 3, N + 8), FILL, dtype=torch.float16, device=gpu)
            out = out_store[:P, :N]
            moe.grouped_gemm(x, scale, ssum, dev(offsets), lin, out, row_src=dev(row_src))
            first = out_store.cpu().numpy().copy()
            _same_f16(first[:P, :N], want, f"epilogue {conv}: against the oracle")
            assert (first[P:] == FILL).all() and (first[:, N:] == FILL).all(), "a row >= P or a guard column was written"
            moe.grouped_gemm(x, scale, ssum, dev(offsets), lin, out, row_src=dev(row_src))
            assert np.array_equal(out_store.cpu().numpy().view(np.uint16), first.view(np.uint16)), "the second launch differs"
            for e in range(2):
                lo, hi = int(offsets[e]), int(offsets[e + 1])
                rows = row_src[lo:hi]
                dense = torch.full((hi - lo, N), FILL, dtype=torch.float16, device=gpu)
                w = lin.expert(e)
                if per_chn:
                    op.gemm_forward_cuda(dev(pr["A"][rows]), w["qweight"], w["s1_scales"], dev(pr["ascales"][rows]), w["s1_szeros"],
                                         dev(pr["a_ssums"][rows]), dense)
                else:
                    op.gemm_forward_cuda(dev(pr["A"][rows]), w["qweight"], w["s2_zeros"], w["s2_scales"], w["s1_scales"],
                                         dev(pr["ascales"][rows]), dense)
                _same_f16(dense.cpu().numpy(), first[lo:hi, :N], f"epilogue {conv}: expert {e} against the dense entry")
    finally:
        lib.qs_set_gemm_epilogue(0)


@_rows("w8a8")
def test_w8a8(gpu, row):
    import qserve_backend.qgemm_w8a8 as op
    pr = cases.row_problem(row)
    M, N = row.M, row.N
    acc = cases.oracle_acc(pr)
    assert np.array_equal(acc.astype(np.int64), cases.problem_acc(*cases.row_problem_key(row)))
    want = cases.oracle_out(pr, acc)
    outs = [torch.full((M + 2, N), FILL, dtype=torch.float16, device=gpu) for _ in range(2)]
    for out in outs:
        op.w8a8_gemm_forward_cuda(dev(pr["A"]), dev(pr["weight"]), dev(pr["wscales"]), dev(pr["ascales"]), out[:M])
    outs = [o.cpu().numpy() for o in outs]
    assert np.isfinite(want).all()
    _same_f16(outs[0][:M], want, "w8a8")
    assert np.array_equal(outs[1].view(np.uint16), outs[0].view(np.uint16)), "the second launch differs from the first"
    assert (outs[0][M:] == FILL).all(), "rows beyond M were written"
