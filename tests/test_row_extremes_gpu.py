"""The activation row kernels (qserve_amd/csrc/fused_small.hip, row_ops.h) at every launch boundary and on extreme rows: the cases of
tests/_row_extreme_cases.py (tests/test_row_extremes_cpu.py proves what they are).

Quantising entries: int8 rows, fp16 scales and fp16 sums are compared AS BITS with oracle.fused in the library's own association
(stats_order = "hip", sum_order = "hip" / "reference"); no element is excluded and nothing is tolerated - the one licence is a NaN's
payload (where the oracle says NaN the device must say NaN).  Pair fusions are compared as bits with the two launches they replace.
Every output lives between guard rows / guard scalars that must keep their sentinel."""
import numpy as np
import pytest
import torch

import _row_extreme_cases as rc
from _helpers import dev, ulp_diff_f16
from oracle import fused, w4a8

pytestmark = pytest.mark.gpu
EPS = 1e-5


# ---- guarded stores -----------------------------------------------------------------------------------------------------------------
class Guarded:
    """[1 + n + 1, *tail] filled with the sentinel; `.t` is the middle (what a launch gets), the first and last slice are the guards."""

    def __init__(self, gpu, n, tail, dtype):
        if dtype == torch.int8:
            self.full = torch.full((n + 2, *tail), rc.SENTINEL_I8, dtype=torch.int8, device=gpu)
        else:
            self.full = torch.full((n + 2, *tail), rc.SENTINEL_F16_BITS, dtype=torch.int16, device=gpu).view(torch.float16)
        self.t = self.full[1:n + 1]
        assert self.t.is_contiguous()

    def _raw(self, t):
        return t if t.dtype == torch.int8 else t.view(torch.int16)

    def guards_intact(self):
        want = rc.SENTINEL_I8 if self.full.dtype == torch.int8 else rc.SENTINEL_F16_BITS
        return bool((self._raw(self.full[0]) == want).all()) and bool((self._raw(self.full[-1]) == want).all())

    def untouched(self):
        want = rc.SENTINEL_I8 if self.full.dtype == torch.int8 else rc.SENTINEL_F16_BITS
        return bool((self._raw(self.full) == want).all())

    def bits(self):
        a = self.t.cpu().numpy()
        return a if a.dtype == np.int8 else a.view(np.uint16)


class Outputs:
    """out int8 [T, H], scale fp16 [T], sum fp16 [T], each guarded."""

    def __init__(self, gpu, T, H):
        self.q, self.sc, self.sm = Guarded(gpu, T, (H,), torch.int8), Guarded(gpu, T, (), torch.float16), Guarded(gpu, T, (), torch.float16)

    def check_guards(self, what, sum_written=True):
        torch.cuda.synchronize()
        assert self.q.guards_intact(), f"{what}: guard row of the int8 output overwritten"
        assert self.sc.guards_intact(), f"{what}: guard scalar of the scales overwritten"
        assert self.sm.guards_intact() if sum_written else self.sm.untouched(), f"{what}: sum store touched beyond what was asked"

    def bits(self):
        return self.q.bits(), self.sc.bits(), self.sm.bits()


def _f16_equal_mod_nan(got_bits, want, what):
    """fp16 bits equal; where they differ both sides are NaN (0 / 0 and inf - inf yield the default NaN of the machine that computes)."""
    want = np.ascontiguousarray(want, np.float16)
    diff = got_bits != want.view(np.uint16)
    if diff.any():
        g = got_bits.view(np.float16)
        assert (np.isnan(g[diff]) & np.isnan(want[diff])).all(), \
            f"{what}: {int(diff.sum())} differ beyond NaN payloads, first {g[diff][:4]} vs {want[diff][:4]} at {np.argwhere(diff)[:4].tolist()}"


def _against_oracle(outs, ora, what, with_sum=True):
    q, sc, sm = outs.bits()
    bad = q != ora[0]
    assert not bad.any(), f"{what}: {int(bad.sum())} int8 values differ, first at {np.argwhere(bad)[:4].tolist()}: " \
                          f"{q[bad][:4]} vs {ora[0][bad][:4]} (pre {ora[-1][bad][:4]})"
    _f16_equal_mod_nan(sc, ora[1], what + ": scale")
    if with_sum:
        _f16_equal_mod_nan(sm, ora[2], what + ": sum")


def _same_bits(a, b, what):
    for x, y, n in zip(a.bits(), b.bits(), ("int8 row", "scale", "sum")):
        assert np.array_equal(x, y), f"{what}: {n} differs at {np.argwhere(x != y)[:4].tolist()}"


def _label(b, i):
    return f"{b.family}[{i}] {b.notes[1] if b.bad_row is not None else b.notes[0]}"


class _Sandwiches:
    """The ordinary rows around an overflow row must come out as when they run alone (rows 0 and 2 of the `alone` batch)."""

    def __init__(self):
        self.alone = None

    def see(self, b, outs, what, extra=None):
        got = [x[[0, 2]] for x in outs.bits()] + ([] if extra is None else [extra[[0, 2]]])
        if b.family == "alone":
            self.alone = got
        elif b.bad_row is not None:
            assert self.alone is not None
            for x, y in zip(got, self.alone):
                assert np.array_equal(x, y), f"{what}: an ordinary row next to the bad row differs from the same row run alone"


@pytest.fixture
def row_sum_order():
    from qserve_amd._lib import lib
    assert lib.qs_get_row_sum_order() == 0

    def set_order(o):
        assert lib.qs_set_row_sum_order(o) == 0
    yield set_order
    lib.qs_set_row_sum_order(0)


def _alone_first(batches):
    return sorted(batches, key=lambda b: b.family != "alone")


# ---- invoke_quant(_fuse_sum) ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", rc.QUANT_WIDTHS)
def test_invoke_quant(gpu, H):
    import qserve_backend.fused_kernels as fk
    print(f"invoke_quant H={H}: quant_kernel<{rc.quant_inst(H)[0]}, {rc.quant_inst(H)[1]}>")
    sw = _Sandwiches()
    for i, b in enumerate(_alone_first(rc.quant_batches(H))):
        what = f"invoke_quant_fuse_sum H={H} {_label(b, i)}"
        x = dev(b.rows)
        T = b.rows.shape[0]
        o = Outputs(gpu, T, H)
        fk.invoke_quant_fuse_sum(o.q.t, x, o.sm.t, o.sc.t)
        o.check_guards(what)
        _against_oracle(o, fused.quant_per_token(b.rows, with_sum=True, sum_order="hip"), what)
        sw.see(b, o, what)
        o2 = Outputs(gpu, T, H)
        fk.invoke_quant(o2.q.t, x, o2.sc.t)
        o2.check_guards(what + " (no sum)", sum_written=False)
        assert np.array_equal(o2.q.bits(), o.q.bits()) and np.array_equal(o2.sc.bits(), o.sc.bits()), what + ": differs without the sum"


# ---- silu_and_mul_quant == silu_and_mul ; invoke_quant ------------------------------------------------------------------------------
@pytest.mark.parametrize("D", rc.QUANT_WIDTHS)
def test_silu_and_mul_quant(gpu, D):
    import qserve_backend.activation_ops as act
    import qserve_backend.fused_kernels as fk
    from qserve_amd import fused as fz
    print(f"silu_and_mul_quant d={D}: silu_mul_quant_kernel<{rc.quant_inst(D)[0]}, {rc.quant_inst(D)[1]}>")
    sw = _Sandwiches()
    for i, b in enumerate(_alone_first(rc.silu_quant_batches(D))):
        what = f"silu_and_mul_quant d={D} {_label(b, i)}"
        gate, up = rc.split_for_silu(b.rows) if b.pair is None else b.pair
        xin = np.concatenate([gate, up], axis=1)
        x = dev(xin)
        T = xin.shape[0]
        o = Outputs(gpu, T, D)
        fz.silu_and_mul_quant(o.q.t, x, o.sc.t, o.sm.t)
        o.check_guards(what)
        # gate = 32 (300 in the overflow row): silu(gate) = gate whatever `exp` returns in its last place, so the oracle's product is the
        # device's, bit for bit (test_silu_and_mul below checks that claim on its own)
        _against_oracle(o, fused.quant_per_token(fused.silu_and_mul(xin), with_sum=True, sum_order="hip"), what)
        sw.see(b, o, what)
        tmp = Guarded(gpu, T, (D,), torch.float16)
        act.silu_and_mul(tmp.t, x)
        p = Outputs(gpu, T, D)
        fk.invoke_quant_fuse_sum(p.q.t, tmp.t, p.sm.t, p.sc.t)
        p.check_guards(what + " (pair)")
        assert tmp.guards_intact()
        _same_bits(o, p, what + ": fusion vs silu_and_mul ; invoke_quant_fuse_sum")
        o2 = Outputs(gpu, T, D)
        fz.silu_and_mul_quant(o2.q.t, x, o2.sc.t, None)
        o2.check_guards(what + " (no sum)", sum_written=False)
        assert np.array_equal(o2.q.bits(), o.q.bits()) and np.array_equal(o2.sc.bits(), o.sc.bits()), what + ": differs without the sum"


# ---- rms_norm_general(_fuse_sum) ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [0, 1], ids=["sum_hip", "sum_reference"])
@pytest.mark.parametrize("H", rc.NORM_WIDTHS)
def test_rms_norm_general(gpu, H, order, row_sum_order):
    import qserve_backend.layernorm_ops as ln
    print(f"rms_norm_general H={H} order={order}: general_norm_quant_kernel<{rc.norm_inst(H, order)[0]}, {rc.norm_inst(H, order)[1]}> with "
          f"input_sum, general_norm_quant_kernel<{rc.norm_inst(H, False)[0]}, False> without")
    row_sum_order(order)
    sw = _Sandwiches()
    for i, b in enumerate(_alone_first(rc.norm_batches(H))):
        what = f"rms_norm_general_fuse_sum H={H} order={order} {_label(b, i)}"
        gamma = rc.default_gamma(H) if b.gamma is None else b.gamma
        x, g = dev(b.rows), dev(gamma)
        T = b.rows.shape[0]
        o = Outputs(gpu, T, H)
        ln.rms_norm_general_fuse_sum(o.q.t, x, g, o.sm.t, o.sc.t, EPS, True)
        o.check_guards(what)
        _against_oracle(o, fused.rms_norm_general(b.rows, gamma, EPS, with_sum=True, sum_order=("hip", "reference")[order],
                                                  stats_order="hip"), what)
        sw.see(b, o, what)
        assert np.array_equal(x.cpu().numpy().view(np.uint16), b.rows.view(np.uint16)), what + ": the input row was written"
        o2 = Outputs(gpu, T, H)
        ln.rms_norm_general(o2.q.t, x, g, o2.sc.t, EPS, True)
        o2.check_guards(what + " (no sum)", sum_written=False)
        assert np.array_equal(o2.q.bits(), o.q.bits()) and np.array_equal(o2.sc.bits(), o.sc.bits()), what + ": differs without the sum"


# ---- add_residual_rms_norm_general == residual_add ; rms_norm_general(_fuse_sum) ----------------------------------------------------
@pytest.mark.parametrize("order", [0, 1], ids=["sum_hip", "sum_reference"])
@pytest.mark.parametrize("H", rc.NORM_WIDTHS)
def test_add_residual_rms_norm_general(gpu, H, order, row_sum_order):
    import qserve_backend.layernorm_ops as ln
    from qserve_amd import fused as fz
    from qserve_amd.decode import residual_add_
    print(f"add_residual_rms_norm_general H={H} order={order}: add_residual_norm_quant_kernel<{rc.add_norm_inst(H, order)}> with input_sum, "
          f"<{rc.add_norm_inst(H, False)}> without")
    row_sum_order(order)
    sw = _Sandwiches()
    for i, b in enumerate(_alone_first(rc.add_norm_batches(H))):
        what = f"add_residual_rms_norm_general H={H} order={order} {_label(b, i)}"
        gamma = rc.default_gamma(H) if b.gamma is None else b.gamma
        hid, delta = rc.split_for_add(b.rows) if b.pair is None else b.pair
        T = hid.shape[0]
        d, g = dev(delta), dev(gamma)
        with np.errstate(over="ignore", invalid="ignore"):
            hsum = hid + delta                                              # the fp16 add (60 000 + 60 000 = inf)
        # the fusion
        h1 = Guarded(gpu, T, (H,), torch.float16)
        h1.t.copy_(dev(hid))
        o = Outputs(gpu, T, H)
        fz.add_residual_rms_norm_general(o.q.t, h1.t, d, g, o.sc.t, EPS, o.sm.t)
        o.check_guards(what)
        assert h1.guards_intact(), what + ": guard row of the residual stream overwritten"
        _f16_equal_mod_nan(h1.bits(), hsum, what + ": residual stream")
        _against_oracle(o, fused.rms_norm_general(hsum, gamma, EPS, with_sum=True, sum_order=("hip", "reference")[order],
                                                  stats_order="hip"), what)
        sw.see(b, o, what, extra=h1.bits())
        # the pair
        h2 = Guarded(gpu, T, (H,), torch.float16)
        h2.t.copy_(dev(hid))
        residual_add_(h2.t, d)
        p = Outputs(gpu, T, H)
        ln.rms_norm_general_fuse_sum(p.q.t, h2.t, g, p.sm.t, p.sc.t, EPS, True)
        p.check_guards(what + " (pair)")
        assert h2.guards_intact() and np.array_equal(h1.bits(), h2.bits()), what + ": residual stream differs from residual_add"
        _same_bits(o, p, what + ": fusion vs residual_add ; rms_norm_general_fuse_sum")
        # without the sum
        h3 = Guarded(gpu, T, (H,), torch.float16)
        h3.t.copy_(dev(hid))
        o3 = Outputs(gpu, T, H)
        fz.add_residual_rms_norm_general(o3.q.t, h3.t, d, g, o3.sc.t, EPS, None)
        o3.check_guards(what + " (no sum)", sum_written=False)
        assert h3.guards_intact() and np.array_equal(h3.bits(), h1.bits())
        assert np.array_equal(d.cpu().numpy().view(np.uint16), delta.view(np.uint16)), what + ": delta was written"
        assert np.array_equal(o3.q.bits(), o.q.bits()) and np.array_equal(o3.sc.bits(), o.sc.bits()), what + ": differs without the sum"


# ---- the K-slice planes entry == host epilogue ; add_residual_rms_norm_general -------------------------------------------------------
@pytest.mark.parametrize("H", rc.PLANES_WIDTHS)
def test_planes_entry_equals_the_pair(gpu, H, row_sum_order):
    from qserve_amd import fused as fz
    from qserve_amd._lib import lib
    T = 5
    ops = rc.planes_operands(T, H)
    t = {k: dev(v) for k, v in ops.items()}
    assert lib.qs_get_gemm_epilogue() == 0
    try:
        for h, ks, mode, ref, fam in rc.planes_cases():
            if h != H:
                continue
            per_group = mode == "per_group"
            what = f"planes H={H} ks={ks} {mode} refsum={ref} {fam}"
            print(f"{what}: add_residual_norm_quant_planes_kernel<{rc.planes_inst(H, ks, per_group, ref)}>")
            planes, acc = rc.planes_problem(T, H, ks, fam)
            if per_group:
                delta = w4a8.epilogue_per_group(acc, ops["wscales"], ops["ascales"])
            else:
                delta = w4a8.epilogue_per_chn(acc, ops["wscales"], ops["ascales"], ops["w_szs"], ops["a_ssums"],
                                              fma=mode == "per_channel_fma")
            row_sum_order(int(ref))
            assert lib.qs_set_gemm_epilogue(int(mode == "per_channel_fma")) == 0
            # the ordinary pair: delta as the GEMM would have stored it, then add + norm + quant
            h1 = Guarded(gpu, T, (H,), torch.float16)
            h1.t.copy_(t["hidden"])
            p = Outputs(gpu, T, H)
            fz.add_residual_rms_norm_general(p.q.t, h1.t, dev(delta), t["gamma"], p.sc.t, EPS, p.sm.t)
            p.check_guards(what + " (pair)")
            # the planes entry; scale / sum are written where the GEMM's ascales / a_ssums live, as the engine passes them
            h2 = Guarded(gpu, T, (H,), torch.float16)
            h2.t.copy_(t["hidden"])
            o = Outputs(gpu, T, H)
            o.sc.t.copy_(t["ascales"])
            pl = dev(planes)
            if per_group:
                fz.add_residual_rms_norm_general_planes(o.q.t, h2.t, pl, t["wscales"], o.sc.t, t["gamma"], o.sc.t, EPS, input_sum=o.sm.t)
            else:
                o.sm.t.copy_(t["a_ssums"])
                fz.add_residual_rms_norm_general_planes(o.q.t, h2.t, pl, t["wscales"], o.sc.t, t["gamma"], o.sc.t, EPS,
                                                        w_szs=t["w_szs"], a_ssums=o.sm.t, input_sum=o.sm.t)
            o.check_guards(what)
            assert h1.guards_intact() and h2.guards_intact()
            assert np.array_equal(h1.bits(), h2.bits()), what + ": residual stream differs"
            _same_bits(o, p, what)
    finally:
        lib.qs_set_gemm_epilogue(0)


# ---- residual_add -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("numel", rc.RESADD_SIZES)
def test_residual_add(gpu, numel):
    from qserve_amd.decode import residual_add_
    print(f"residual_add numel={numel}: {rc.resadd_trips(numel)} trip(s) of the grid-stride loop")
    g = torch.Generator(device=gpu).manual_seed(numel % 1000003)
    a = Guarded(gpu, 1, (numel + 64,), torch.float16)                  # 64 sentinel values behind the last element, too
    tail = a.t[0, numel:].clone()
    x = a.t[0, :numel]
    x.copy_((torch.randn((numel,), device=gpu, generator=g) * 3).half())
    b = (torch.randn((numel,), device=gpu, generator=g) * 2).half()
    for p, v in ((0, 60000.0), (numel - 1, -60000.0), (numel // 2, 65504.0), (7, float("inf"))):     # sums that overflow, at both ends
        x[p] = v
        b[p] = v
    x[1], b[1] = 0.0, -0.0
    want = x + b
    assert torch.isinf(want[[0, numel - 1, numel // 2]]).all()
    residual_add_(x, b)
    torch.cuda.synchronize()
    assert torch.equal(x.view(torch.int16), want.view(torch.int16))
    assert a.guards_intact() and torch.equal(a.t[0, numel:].view(torch.int16), tail.view(torch.int16)), "written behind the last element"


# ---- silu_and_mul -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", rc.SILU_WIDTHS)
def test_silu_and_mul(gpu, d):
    import qserve_backend.activation_ops as act
    print(f"silu_and_mul d={d}: {rc.silu_trips(d)} trip(s) of the column loop")
    x = rc.gaussian(3, 2 * d, 31, 2.0)
    o = Guarded(gpu, 3, (d,), torch.float16)
    act.silu_and_mul(o.t, dev(x))
    torch.cuda.synchronize()
    assert o.guards_intact()
    # the bar of tests/test_fused_gpu.py::test_rms_norm_and_silu: expf differs by an fp32 ulp between libraries - half(silu) can flip by
    # one ulp, the product by one more
    assert ulp_diff_f16(o.t.cpu().numpy(), fused.silu_and_mul(x)).max() <= 2
    # the regions where the result does not depend on exp's last place (_row_extreme_cases.SILU_GATES): 0 ulp, the sign of zero and
    # inf / NaN included.  Rests on v_rcp_f32(1.0) == 1.0 and v_exp_f32 of an argument >= 128 being +inf.
    xr = rc.silu_regions(d)
    o = Guarded(gpu, 3, (d,), torch.float16)
    act.silu_and_mul(o.t, dev(xr))
    torch.cuda.synchronize()
    assert o.guards_intact()
    _f16_equal_mod_nan(o.bits(), fused.silu_and_mul(xr), f"silu_and_mul d={d} regions")


# ---- rms_norm -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", rc.RMS_WIDTHS)
def test_rms_norm(gpu, H):
    import qserve_backend.layernorm_ops as ln
    print(f"rms_norm H={H}: {-(-H // rc.ROW)} trip(s) of the row loop")
    w = rc.default_gamma(H)
    x = rc.gaussian(4, H, 32)
    o = Guarded(gpu, 4, (H,), torch.float16)
    ln.rms_norm(o.t, dev(x), dev(w), EPS)
    torch.cuda.synchronize()
    assert o.guards_intact()
    # the bar of tests/test_fused_gpu.py::test_rms_norm_and_silu: half(x * rstd) can flip by one ulp with the fp32 summation order of the
    # variance, the product by one more
    assert ulp_diff_f16(o.t.cpu().numpy(), fused.rms_norm(x, w, EPS)).max() <= 2
    # |x| = 2 everywhere: every partial sum of squares is exact, the variance is 4 in any order - 0 ulp.  Rests on 1.0f / sqrtf() being
    # correctly rounded in this build.
    xe = rc.rms_exact_rows(H)
    o = Guarded(gpu, 3, (H,), torch.float16)
    ln.rms_norm(o.t, dev(xe), dev(w), EPS)
    torch.cuda.synchronize()
    assert o.guards_intact()
    assert np.array_equal(o.bits(), fused.rms_norm(xe, w, EPS).view(np.uint16)), \
        int(ulp_diff_f16(o.t.cpu().numpy(), fused.rms_norm(xe, w, EPS)).max())


# ---- what the tables above launch ---------------------------------------------------------------------------------------------------
def test_every_instantiation_is_launched(gpu):
    """The instantiation each case above selects, by the launchers' rules as tests/test_row_extremes_cpu.py re-derived them from the
    sources (the library is not asked): together they are every instantiation the launchers can select."""
    got = dict(
        quant_kernel={rc.quant_inst(h) for h in rc.QUANT_WIDTHS},
        silu_mul_quant_kernel={rc.quant_inst(h) for h in rc.QUANT_WIDTHS},
        general_norm_quant_kernel={rc.norm_inst(h, r) for h in rc.NORM_WIDTHS for r in (False, True)},
        add_residual_norm_quant_kernel={rc.add_norm_inst(h, r) for h in rc.NORM_WIDTHS for r in (False, True)},
        add_residual_norm_quant_planes_kernel={rc.planes_inst(h, ks, m == "per_group", r) for h, ks, m, r, _ in rc.planes_cases()})
    for k, v in got.items():
        print(f"{k}: {len(v)} instantiations")
        for inst in sorted(v):
            print(f"    <{', '.join(str(x).lower() if isinstance(x, bool) else str(x) for x in inst)}>")
    assert got["quant_kernel"] == rc.ALL_QUANT_INST and got["silu_mul_quant_kernel"] == rc.ALL_QUANT_INST
    assert got["general_norm_quant_kernel"] == rc.ALL_NORM_INST
    assert got["add_residual_norm_quant_kernel"] == rc.ALL_ADD_NORM_INST
    assert got["add_residual_norm_quant_planes_kernel"] == rc.ALL_PLANES_INST
