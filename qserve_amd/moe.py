"""Mixture-of-experts MLPs over the W4A8 linears (extension; NOT part of the reference's `qserve_backend` surface: the reference's Mixtral
block, qserve/modeling/models/mixtral_w4a8_unpad.py, spells the pipeline out and raises before routing - its kernels were never released).

    route        fp16 router logits [T, E] -> per token the k experts of the largest logits (value descending, expert index ascending), their
                 softmax weights, and the stable expert sort of the T k pairs: offsets, source tokens, sorted positions - all on the device
    grouped_gemm out[p] = W[e(p)] x[row_src[p]] for every sorted position p, W the stacked expert weights of a `MoELinear`
    combine      out[t] = half(sum_j weights[t, j] * float(y[pair_pos[t, j]])), float32, j ascending
    moe_mlp      route -> grouped gate_up -> fused.silu_and_mul_quant over the T k sorted rows -> grouped down -> combine
    MoELinear    the stacked expert weights: qweight [E, N, K/2], s1_scales [E, N], s1_szeros [E, N] | s2_scales / s2_zeros [E, K/128, N]

include/qserve_amd.h (`qs_moe_route`, `qs_w4a8_per_*_moe_gemm`, `qs_moe_combine`) has the rules; a numpy restatement is tests/_moe_cases.py.
Backed by qserve_amd/csrc/moe_route.hip and gemm_w4a8_moe.hip.  DecodeEngine runs `moe_mlp` in place of the dense MLP for a config with
`experts` / `experts_per_token`; it looks the function up per call, so a test can wrap it."""
import ctypes

import torch

from . import fused as fusedmod
from .backend._util import check, expect, guard, lib, ptr, stream

MAX_EXPERTS, MAX_TOP_K = 64, 8


def _same_device(what, first, *rest):
    if any(t is not None and t.device != first.device for t in rest):
        raise RuntimeError(f"{what}: every tensor must be on {first.device}")


def _route_shape(what, T, E, k):
    if not (1 <= E <= MAX_EXPERTS and 1 <= k <= min(E, MAX_TOP_K)):
        raise RuntimeError(f"{what}: E={E} experts (1 .. {MAX_EXPERTS}), k={k} (1 .. min(E, {MAX_TOP_K}))")
    if T * k > 1 << 24:
        raise RuntimeError(f"{what}: T * k = {T * k} pairs (<= 2^24)")


def route_workspace_bytes(T, E, k):
    """Bytes of the workspace one `route` call of these sizes needs (qs_moe_route_workspace)."""
    n = lib.qs_moe_route_workspace(int(T), int(E), int(k))
    check(0 if n >= 0 else int(n), "moe.route_workspace_bytes")
    return int(n)


def route_buffers(T, E, k, device):
    """The five outputs of `route` and its workspace, for T tokens: (expert_ids, weights, expert_offsets, pair_token, pair_pos, workspace)."""
    i32 = dict(dtype=torch.int32, device=device)
    return (torch.empty((T, k), **i32), torch.empty((T, k), dtype=torch.float32, device=device), torch.empty((E + 1,), **i32),
            torch.empty((T * k,), **i32), torch.empty((T, k), **i32),
            torch.empty((max(route_workspace_bytes(T, E, k), 16),), dtype=torch.uint8, device=device))


def route(logits, k, out=None):
    """logits fp16 [T, E] (unit column stride, rows may be padded), finite -> (expert_ids int32 [T, k], weights float32 [T, k],
    expert_offsets int32 [E + 1], pair_token int32 [T k], pair_pos int32 [T, k]), on the device, nothing read back (qs_moe_route has the
    rule).  `out`: `route_buffers(T, E, k, device)` (None: fresh ones)."""
    what = "moe.route"
    expect(logits, torch.float16, "logits", contiguous=False)
    if logits.dim() != 2 or (logits.size(1) > 1 and logits.stride(1) != 1):
        raise RuntimeError(f"{what}: logits must be [T, E] with a unit column stride, got {tuple(logits.shape)}, strides {logits.stride()}")
    T, E = logits.shape
    k = int(k)
    _route_shape(what, T, E, k)
    stride = max(logits.stride(0), E) if T <= 1 else logits.stride(0)
    if stride < E:
        raise RuntimeError(f"{what}: the row stride of logits ({stride}) must be >= E={E}")
    if out is None:
        out = route_buffers(T, E, k, logits.device)
    ids, w, offs, ptok, ppos, ws = out
    for t, dt, name, shape in ((ids, torch.int32, "expert_ids", (T, k)), (w, torch.float32, "weights", (T, k)),
                               (offs, torch.int32, "expert_offsets", (E + 1,)), (ptok, torch.int32, "pair_token", (T * k,)),
                               (ppos, torch.int32, "pair_pos", (T, k))):
        expect(t, dt, name)
        if tuple(t.shape) != shape:
            raise RuntimeError(f"{what}: {name} must be {shape}, got {tuple(t.shape)}")
    need = route_workspace_bytes(T, E, k)
    if not isinstance(ws, torch.Tensor) or not ws.is_cuda or not ws.is_contiguous() or ws.numel() * ws.element_size() < need:
        raise RuntimeError(f"{what}: workspace must be a contiguous device tensor of at least {need} bytes")
    _same_device(what, logits, ids, w, offs, ptok, ppos, ws)
    with guard(logits):
        check(lib.qs_moe_route(ptr(logits), stride, T, E, k, ptr(ids), ptr(w), ptr(offs), ptr(ptok), ptr(ppos), ptr(ws),
                               ws.numel() * ws.element_size(), stream()), what)
    return ids, w, offs, ptok, ppos


def gemm_plan(P, E, N, K):
    """(m-tiles per workgroup, waves per workgroup, row blocks launched, 64-channel units) of a grouped GEMM (qs_moe_gemm_plan): a pure
    function of the sizes, no device access."""
    plan = (ctypes.c_int * 4)()
    check(lib.qs_moe_gemm_plan(int(P), int(E), int(N), int(K), plan), "moe.gemm_plan")
    return tuple(plan)


class MoELinear:
    """The E expert weights of one projection, each in the reference's packed W4A8 layout, stacked: qweight int8 [E, n, k/2], s1_scales
    fp16 [E, n], and s1_szeros fp16 [E, n] (per-channel, group_size -1) or s2_scales / s2_zeros int8 [E, k/128, n] (group_size 128).
    Built from synthetic random tensors (the ranges of decode.W4A8Linear) or from checkpoint tensors (`from_tensors`, fed by
    qserve_amd.loader.load_mixtral_w4a8)."""

    def __init__(self, experts, n, k, group_size, device, gen):
        self.experts, self.n, self.k, self.group_size = experts, n, k, group_size
        E = experts
        self.qweight = torch.randint(-128, 128, (E, n, k // 2), dtype=torch.int8, device=device, generator=gen)
        self.s1_scales = (torch.rand((E, n), device=device, generator=gen) * 0.004 + 0.001).half()
        if group_size == -1:
            z = torch.randint(0, 16, (E, n), device=device, generator=gen).half()
            self.s1_szeros = (z * self.s1_scales).half()
        else:
            self.s2_scales = torch.randint(1, 9, (E, k // 128, n), dtype=torch.int8, device=device, generator=gen)
            zz = torch.randint(0, 16, (E, k // 128, n), device=device, generator=gen).to(torch.int16)
            self.s2_zeros = (-(zz * self.s2_scales.to(torch.int16))).to(torch.int8)

    @classmethod
    def from_tensors(cls, d, group_size):
        """d: {"qweight", "s1_scales", "s1_szeros" | ("s2_scales", "s2_zeros")}, stacked over experts, already on the device."""
        self = cls.__new__(cls)
        self.experts, self.n, self.k, self.group_size = d["qweight"].shape[0], d["qweight"].shape[1], d["qweight"].shape[2] * 2, group_size
        self.qweight, self.s1_scales = d["qweight"], d["s1_scales"]
        assert tuple(self.s1_scales.shape) == (self.experts, self.n)
        if group_size == -1:
            self.s1_szeros = d["s1_szeros"]
            assert tuple(self.s1_szeros.shape) == (self.experts, self.n)
        else:
            self.s2_scales, self.s2_zeros = d["s2_scales"], d["s2_zeros"]
            assert tuple(self.s2_scales.shape) == tuple(self.s2_zeros.shape) == (self.experts, self.k // 128, self.n)
        return self

    def tensors(self):
        names = ("qweight", "s1_scales", "s1_szeros") if self.group_size == -1 else ("qweight", "s1_scales", "s2_scales", "s2_zeros")
        return {n: getattr(self, n) for n in names}

    def expert(self, e):
        """Expert e's tensors in the form decode.W4A8Linear.from_tensors takes (views)."""
        return {n: t[e] for n, t in self.tensors().items()}


def grouped_gemm(x, x_scale, x_sum, expert_offsets, lin, out, row_src=None):
    """out[p, :] = lin's expert e(p) applied to x[row_src[p], :] for every sorted position p < P = out's rows, e(p) the expert whose range
    of `expert_offsets` int32 [E + 1] holds p; row_src int32 [P] (None: x row p).  x int8 [rows, K] and out fp16 [P, N] may have padded
    rows (strides multiples of 16 and 8); x_scale (and, for per-channel weights, x_sum) fp16 [rows] belong to the SOURCE row.  Bit-identical
    to the dense GEMM op on expert e's tensors and that row.  -> out."""
    what = "moe.grouped_gemm"
    expect(x, torch.int8, "x", contiguous=False)
    expect(out, torch.float16, "out", contiguous=False)
    expect(x_scale, torch.float16, "x_scale")
    expect(expert_offsets, torch.int32, "expert_offsets")
    per_group = lin.group_size != -1
    if not per_group:
        if x_sum is None:
            raise RuntimeError(f"{what}: per-channel weights need x_sum (the rows' a_ssums)")
        expect(x_sum, torch.float16, "x_sum")
    if row_src is not None:
        expect(row_src, torch.int32, "row_src")
    for t, name in ((x, "x"), (out, "out")):
        if t.dim() != 2 or (t.size(1) > 1 and t.stride(1) != 1):
            raise RuntimeError(f"{what}: {name} must be [rows, n] with a unit column stride, got {tuple(t.shape)}, strides {t.stride()}")
    (rows, K), (P, N), E = x.shape, out.shape, lin.experts
    if (N, K) != (lin.n, lin.k):
        raise RuntimeError(f"{what}: x has K={K}, out N={N}; the experts are [{lin.n}, {lin.k}]")
    if not 1 <= E <= MAX_EXPERTS or tuple(expert_offsets.shape) != (E + 1,):
        raise RuntimeError(f"{what}: E={E} experts (1 .. {MAX_EXPERTS}) need expert_offsets [{E + 1}], got {tuple(expert_offsets.shape)}")
    if K < 128 or K % 128 != 0 or N % 64 != 0 or N < 64:
        raise RuntimeError(f"{what}: K={K} must be a multiple of 128, N={N} a multiple of 64")
    if rows < 1 or tuple(x_scale.shape) != (rows,) or (not per_group and tuple(x_sum.shape) != (rows,)):
        raise RuntimeError(f"{what}: x has {rows} rows (>= 1), x_scale {tuple(x_scale.shape)}" +
                           ("" if per_group else f", x_sum {tuple(x_sum.shape)}"))
    if row_src is None and rows < P:
        raise RuntimeError(f"{what}: without row_src x needs at least P={P} rows, it has {rows}")
    if row_src is not None and tuple(row_src.shape) != (P,):
        raise RuntimeError(f"{what}: row_src must be [{P}], got {tuple(row_src.shape)}")
    x_stride = max(x.stride(0), K) if rows <= 1 else x.stride(0)
    out_stride = max(out.stride(0), N) if P <= 1 else out.stride(0)
    if x_stride < K or x_stride % 16 != 0 or out_stride < N or out_stride % 8 != 0:
        raise RuntimeError(f"{what}: the row strides of x ({x_stride}: >= K, a multiple of 16) and out ({out_stride}: >= N, a multiple of 8)")
    for name, t in lin.tensors().items():
        expect(t, t.dtype, name)
    _same_device(what, out, x, x_scale, x_sum, expert_offsets, row_src, *lin.tensors().values())
    if P == 0:
        return out
    with guard(out):
        if per_group:
            check(lib.qs_w4a8_per_group_moe_gemm(ptr(x), x_stride, rows, ptr(row_src), ptr(expert_offsets), ptr(lin.qweight), ptr(lin.s2_zeros),
                                                 ptr(lin.s2_scales), ptr(lin.s1_scales), ptr(x_scale), ptr(out), out_stride, P, E, N, K,
                                                 stream()), what)
        else:
            check(lib.qs_w4a8_per_chn_moe_gemm(ptr(x), x_stride, rows, ptr(row_src), ptr(expert_offsets), ptr(lin.qweight), ptr(lin.s1_scales),
                                               ptr(x_scale), ptr(lin.s1_szeros), ptr(x_sum), ptr(out), out_stride, P, E, N, K, stream()),
                  what)
    return out


def combine(out, y, weights, pair_pos):
    """out[t, :] = half(sum_j weights[t, j] * float(y[pair_pos[t, j], :])): float32, j ascending, every multiply and add rounded on its own,
    one rounding to fp16 (qs_moe_combine).  out fp16 [T, N], y fp16 [T k, N] (rows may be padded: strides multiples of 8), weights float32
    and pair_pos int32 [T, k].  -> out."""
    what = "moe.combine"
    expect(out, torch.float16, "out", contiguous=False)
    expect(y, torch.float16, "y", contiguous=False)
    expect(weights, torch.float32, "weights")
    expect(pair_pos, torch.int32, "pair_pos")
    for t, name in ((out, "out"), (y, "y")):
        if t.dim() != 2 or (t.size(1) > 1 and t.stride(1) != 1):
            raise RuntimeError(f"{what}: {name} must be [rows, N] with a unit column stride, got {tuple(t.shape)}, strides {t.stride()}")
    T, N = out.shape
    if weights.dim() != 2 or weights.size(0) != T or not 1 <= weights.size(1) <= MAX_TOP_K or pair_pos.shape != weights.shape:
        raise RuntimeError(f"{what}: weights and pair_pos must be [T={T}, k] with k in 1 .. {MAX_TOP_K}, got {tuple(weights.shape)}, "
                           f"{tuple(pair_pos.shape)}")
    k = weights.size(1)
    if tuple(y.shape) != (T * k, N) or N < 64 or N % 64 != 0:
        raise RuntimeError(f"{what}: y must be [T k = {T * k}, N = {N}], N a multiple of 64, got {tuple(y.shape)}")
    out_stride = max(out.stride(0), N) if T <= 1 else out.stride(0)
    y_stride = max(y.stride(0), N) if T * k <= 1 else y.stride(0)
    if out_stride < N or out_stride % 8 != 0 or y_stride < N or y_stride % 8 != 0:
        raise RuntimeError(f"{what}: the row strides of out ({out_stride}) and y ({y_stride}) must be >= N and multiples of 8")
    _same_device(what, out, y, weights, pair_pos)
    if T == 0:
        return out
    with guard(out):
        check(lib.qs_moe_combine(ptr(out), out_stride, ptr(y), y_stride, ptr(weights), ptr(pair_pos), T, k, N, stream()), what)
    return out


def mlp_buffers(T, experts, k, hidden, inter, device):
    """What `moe_mlp` writes for T token rows: `route_buffers` under "route", and for the T k sorted rows the grouped gate_up output fp16
    [T k, 2 inter], its quantised silu * mul int8 [T k, inter] with scales / sums fp16 [T k], and the grouped down output fp16 [T k, hidden]."""
    P, f16 = T * k, torch.float16
    return dict(route=route_buffers(T, experts, k, device), gate_up=torch.empty((P, 2 * inter), dtype=f16, device=device),
                q_mlp=torch.empty((P, inter), dtype=torch.int8, device=device), q_scale=torch.empty((P,), dtype=f16, device=device),
                q_sum=torch.empty((P,), dtype=f16, device=device), y=torch.empty((P, hidden), dtype=f16, device=device))


def slice_buffers(bufs, T, k):
    """`mlp_buffers` of more rows, cut to T rows (views; the offsets and the workspace are shared)."""
    ids, w, offs, ptok, ppos, ws = bufs["route"]
    P = T * k
    out = {name: bufs[name][:P] for name in ("gate_up", "q_mlp", "q_scale", "q_sum", "y")}
    out["route"] = (ids[:T], w[:T], offs, ptok[:P], ppos[:T], ws)
    return out


def moe_mlp(out, x, x_scale, x_sum, logits, k, gate_up, down, bufs):
    """The sparse MLP of a Mixtral layer on T rows (mixtral_w4a8_unpad.py:279-374): x int8 [T, hidden] with x_scale (and x_sum, per-channel
    weights) fp16 [T]: the quantised normed rows; logits fp16 [T, E]: the router's output on the un-quantised normed rows; gate_up: MoELinear
    [E, 2 inter, hidden] (w1 stacked over w3), down: MoELinear [E, hidden, inter] (w2).  route -> grouped gate_up on the gathered rows ->
    silu_and_mul + quant over the T k sorted rows -> grouped down -> weighted un-permute into out fp16 [T, hidden].  `bufs`:
    `mlp_buffers` of exactly T rows.  Nothing leaves the device.  -> out."""
    ids, w, offs, ptok, ppos = route(logits, k, out=bufs["route"])
    grouped_gemm(x, x_scale, x_sum, offs, gate_up, bufs["gate_up"], row_src=ptok)
    per_chn = down.group_size == -1
    fusedmod.silu_and_mul_quant(bufs["q_mlp"], bufs["gate_up"], bufs["q_scale"], bufs["q_sum"] if per_chn else None)
    grouped_gemm(bufs["q_mlp"], bufs["q_scale"], bufs["q_sum"] if per_chn else None, offs, down, bufs["y"])
    return combine(out, bufs["y"], w, ppos)
