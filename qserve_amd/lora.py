"""LoRA adapters over the W4A8 linears (extension; NOT part of the reference's `qserve_backend` surface): every sequence of a batch runs
under its own low-rank adapter, or under none.  A delta cannot be merged into 4-bit packed weights, so it is applied next to the base
GEMM, per row, on the quantised activations that GEMM read - capturable in a hipGraph, the adapter ids in a device tensor.

    lora_rows   out[t, :] += scaling[a] * B[a] (A[a] x[t]) in place, a = seq_adapter[t // rows_per_seq]; rows of an id outside
                0 .. slots-1 are neither read nor written.
    LoraTable   the A / B tensors of every layer and linear for `slots` adapters of rank <= `rank`, filled from PEFT-named tensors
                (`load`) in the row order qserve_amd.loader fuses the base weights in, zeroed again by `unload`.

include/qserve_amd.h (`qs_lora_rows`) has the rule; a float64 numpy restatement is tests/_lora_cases.py.  Backed by
qserve_amd/csrc/lora_rows.hip.  DecodeEngine.enable_lora / load_lora / set_lora put it behind the four linears of every layer."""
import re

import torch

from .backend._util import check, expect, guard, lib, ptr, stream
from .drafting import _typed

RANKS = (8, 16, 32, 64)
MAX_SEGMENTS = 3
LINEARS = ("qkv", "o", "gate_up", "down")
_PEFT_NAME = re.compile(r"(?:^|\.)layers\.(\d+)\.(?:self_attn|mlp)\.(q|k|v|o|gate|up|down)_proj\.lora_(A|B)(?:\.[^.]+)?\.weight$")
# PEFT module -> (the linear it belongs to, its segment there): the order loader.load_llama_w4a8 fuses q / k / v and gate / up in
_MODULES = dict(q=("qkv", 0), k=("qkv", 1), v=("qkv", 2), o=("o", 0), gate=("gate_up", 0), up=("gate_up", 1), down=("down", 0))


def workspace_bytes(T, K, r, nseg):
    """Bytes of the float32 workspace one `lora_rows` call of these sizes needs (qs_lora_rows_workspace)."""
    n = lib.qs_lora_rows_workspace(int(T), int(K), int(r), int(nseg))
    check(0 if n >= 0 else int(n), "lora.workspace_bytes")
    return int(n)


def lora_rows(out, x, x_scale, A, B, scaling, seq_adapter, rows_per_seq, seg_ends, workspace=None):
    """out[t, n] = fp16(out[t, n] + scaling[a] * sum_j B[a, n, j] * t_j) in place, t_j = x_scale[t] * sum_k A[a, g r + j, k] * x[t, k] in
    float32, for every row t whose sequence's adapter a = seq_adapter[t // rows_per_seq] lies in 0 .. slots-1; g: the segment of column
    n.  out fp16 [T, N]; x int8 [T, K] and x_scale fp16 [T]: the quantised activations the base GEMM read; A fp16 [slots, nseg * r, K];
    B fp16 [slots, N, r]; scaling float32 [slots]; seq_adapter int32 [T / rows_per_seq]; seg_ends: the nseg (1 .. 3) ascending segment
    ends, multiples of 64, the last one N.  r in 8, 16, 32, 64; K a multiple of 128, N of 64; out and x may have padded rows (strides
    multiples of 8 and 16).  `workspace`: a contiguous device tensor of at least workspace_bytes(T, K, r, nseg) bytes (None: a fresh
    one).  -> out."""
    what = "lora.lora_rows"
    _typed(out, torch.float16, "out")
    _typed(x, torch.int8, "x")
    _typed(x_scale, torch.float16, "x_scale")
    _typed(A, torch.float16, "A")
    _typed(B, torch.float16, "B")
    _typed(scaling, torch.float32, "scaling")
    _typed(seq_adapter, torch.int32, "seq_adapter")
    for t, name in ((out, "out"), (x, "x")):
        if t.dim() != 2 or (t.size(1) > 1 and t.stride(1) != 1):
            raise RuntimeError(f"{what}: {name} must be [T, n] with a unit column stride, got {tuple(t.shape)}, strides {t.stride()}")
    (T, N), K = out.shape, x.size(1)
    if x.size(0) != T or x_scale.dim() != 1 or x_scale.numel() != T:
        raise RuntimeError(f"{what}: out has {T} rows, x {x.size(0)}, x_scale {tuple(x_scale.shape)}")
    seg_ends = [int(e) for e in seg_ends]
    nseg = len(seg_ends)
    if not 1 <= nseg <= MAX_SEGMENTS or seg_ends != sorted(set(seg_ends)) or seg_ends[0] <= 0 or any(e % 64 for e in seg_ends) or \
            seg_ends[-1] != N:
        raise RuntimeError(f"{what}: seg_ends={seg_ends} must be 1 .. {MAX_SEGMENTS} ascending multiples of 64, the last one N={N}")
    if B.dim() != 3 or B.size(1) != N or B.size(2) not in RANKS:
        raise RuntimeError(f"{what}: B must be [slots, N={N}, r] with r in {RANKS}, got {tuple(B.shape)}")
    slots, r = B.size(0), B.size(2)
    if slots < 1 or tuple(A.shape) != (slots, nseg * r, K) or tuple(scaling.shape) != (slots,):
        raise RuntimeError(f"{what}: A must be [{slots}, {nseg * r}, K={K}] and scaling [{slots}], got {tuple(A.shape)}, "
                           f"{tuple(scaling.shape)}")
    if K < 128 or K % 128 != 0 or N % 64 != 0:
        raise RuntimeError(f"{what}: K={K} must be a multiple of 128, N={N} a multiple of 64")
    rows_per_seq = int(rows_per_seq)
    if rows_per_seq < 1 or T % rows_per_seq != 0 or tuple(seq_adapter.shape) != (T // rows_per_seq,):
        raise RuntimeError(f"{what}: T={T} must be a multiple of rows_per_seq={rows_per_seq} (>= 1) and seq_adapter hold one id per "
                           f"sequence, got {tuple(seq_adapter.shape)}")
    out_stride = max(out.stride(0), N) if T <= 1 else out.stride(0)
    x_stride = max(x.stride(0), K) if T <= 1 else x.stride(0)
    if out_stride < N or out_stride % 8 != 0 or x_stride < K or x_stride % 16 != 0:
        raise RuntimeError(f"{what}: the row strides of out ({out_stride}: >= N, a multiple of 8) and x ({x_stride}: >= K, a multiple of 16)")
    expect(out, torch.float16, "out", contiguous=False)
    expect(x, torch.int8, "x", contiguous=False)
    for t, name in ((x_scale, "x_scale"), (A, "A"), (B, "B"), (scaling, "scaling"), (seq_adapter, "seq_adapter")):
        expect(t, t.dtype, name)
    if any(t.device != out.device for t in (x, x_scale, A, B, scaling, seq_adapter)):
        raise RuntimeError(f"{what}: every tensor must be on {out.device}")
    need = workspace_bytes(T, K, r, nseg)
    if workspace is None:
        workspace = torch.empty((max(need, 16),), dtype=torch.uint8, device=out.device)
    if not isinstance(workspace, torch.Tensor) or not workspace.is_cuda or workspace.device != out.device or not workspace.is_contiguous() or \
            workspace.numel() * workspace.element_size() < need:
        raise RuntimeError(f"{what}: workspace must be a contiguous tensor of at least {need} bytes on {out.device}")
    if T == 0:
        return out
    e = seg_ends + [0] * (MAX_SEGMENTS - nseg)
    with guard(out):
        check(lib.qs_lora_rows(ptr(out), out_stride, ptr(x), x_stride, ptr(x_scale), ptr(A), ptr(B), ptr(scaling), ptr(seq_adapter), slots, T,
                               K, N, r, rows_per_seq, nseg, e[0], e[1], e[2], ptr(workspace), workspace.numel() * workspace.element_size(),
                               stream()), what)
    return out


def linear_shapes(cfg):
    """name -> (K, N, segment ends) of the four linears of a layer of `cfg` (qserve_amd.decode configs), fused as the loader fuses them:
    q | k | v and gate | up.  Heads are 128 wide, whatever `hidden` is (the engine's rule)."""
    hid, H, Hkv, inter = cfg["hidden"], cfg["heads"], cfg["kv_heads"], cfg["inter"]
    hd = 128
    return dict(qkv=(hid, (H + 2 * Hkv) * hd, (H * hd, (H + Hkv) * hd, (H + 2 * Hkv) * hd)), o=(H * hd, hid, (hid,)),
                gate_up=(hid, 2 * inter, (inter, 2 * inter)), down=(inter, hid, (hid,)))


class LoraTable:
    """`slots` adapters of rank <= `rank` for a model of `cfg`: per layer and linear ("qkv", "o", "gate_up", "down") A fp16
    [slots, nseg * rank, K] - segment g of a fused linear owns rows g * rank .. g * rank + rank - 1 - and B fp16 [slots, N, rank], plus
    one scaling float32 [slots].  Starts zeroed: an empty slot adds exact zeros."""

    def __init__(self, cfg, slots, rank, device):
        slots, rank = int(slots), int(rank)
        if slots < 1 or rank not in RANKS:
            raise ValueError(f"LoraTable: slots={slots} (>= 1), rank={rank} (one of {RANKS})")
        self.cfg, self.slots, self.rank, self.device = cfg, slots, rank, torch.device(device)
        self.shapes = linear_shapes(cfg)
        self.layers = []
        for _ in range(cfg["layers"]):
            self.layers.append({name: (torch.zeros((slots, len(ends) * rank, K), dtype=torch.float16, device=self.device),
                                       torch.zeros((slots, N, rank), dtype=torch.float16, device=self.device))
                                for name, (K, N, ends) in self.shapes.items()})
        self.scaling = torch.zeros((slots,), dtype=torch.float32, device=self.device)

    def _slot(self, slot, what):
        slot = int(slot)
        if not 0 <= slot < self.slots:
            raise ValueError(f"LoraTable.{what}: slot={slot} (0 .. {self.slots - 1})")
        return slot

    def load(self, slot, tensors, alpha):
        """Fill `slot` from `tensors`, a dict under PEFT's names - `...layers.{i}.self_attn.{q,k,v,o}_proj.lora_{A,B}.weight`,
        `...mlp.{gate,up,down}_proj.lora_{A,B}.weight` (any prefix; an adapter name between `lora_A` and `weight` is accepted), lora_A
        [r', K] and lora_B [N, r'] - and set scaling[slot] = alpha / r'.  One r' <= rank for the whole adapter; a smaller one is
        zero-padded, which is exact.  Modules the dict does not name stay zero; keys of another form are ignored.  Refused, with the slot
        unchanged: r' > rank, a wrong shape, an A without its B (or the reverse), a layer that does not exist."""
        slot = self._slot(slot, "load")
        found = {}
        for name, t in tensors.items():
            m = _PEFT_NAME.search(name)
            if m is None:
                continue
            li, mod, ab = int(m.group(1)), m.group(2), m.group(3)
            if li >= len(self.layers):
                raise ValueError(f"LoraTable.load: {name}: the model has {len(self.layers)} layers")
            if not isinstance(t, torch.Tensor) or t.dim() != 2:
                raise ValueError(f"LoraTable.load: {name} must be a 2-d tensor")
            found.setdefault((li, mod), {})[ab] = (name, t)
        if not found:
            raise ValueError("LoraTable.load: no `...layers.N.(self_attn|mlp).X_proj.lora_(A|B).weight` tensor in the dict")
        ranks, hd = set(), self.cfg["hidden"] // self.cfg["heads"]
        for (li, mod), ab in found.items():
            if set(ab) != {"A", "B"}:
                raise ValueError(f"LoraTable.load: layer {li} {mod}_proj has lora_{'A' if 'A' in ab else 'B'} only")
            lin, g = _MODULES[mod]
            K, _, ends = self.shapes[lin]
            n = ends[g] - (ends[g - 1] if g else 0)
            (na, a), (nb, b) = ab["A"], ab["B"]
            r1 = a.size(0)
            if a.size(1) != K or tuple(b.shape) != (n, r1):
                raise ValueError(f"LoraTable.load: {na} {tuple(a.shape)} / {nb} {tuple(b.shape)} must be [r, {K}] / [{n}, r]")
            ranks.add(r1)
        if len(ranks) != 1:
            raise ValueError(f"LoraTable.load: one rank per adapter (scaling = alpha / r), got {sorted(ranks)}")
        r1 = ranks.pop()
        if not 1 <= r1 <= self.rank:
            raise ValueError(f"LoraTable.load: the adapter has rank {r1}, the table holds rank <= {self.rank}")
        self.unload(slot)
        for (li, mod), ab in found.items():
            lin, g = _MODULES[mod]
            ends = self.shapes[lin][2]
            n0 = ends[g - 1] if g else 0
            A, B = self.layers[li][lin]
            A[slot, g * self.rank:g * self.rank + r1].copy_(ab["A"][1].to(torch.float16))
            B[slot, n0:ends[g], :r1].copy_(ab["B"][1].to(torch.float16))
        self.scaling[slot] = float(alpha) / r1

    def unload(self, slot):
        """Zero `slot`: its rows then add exact zeros."""
        slot = self._slot(slot, "unload")
        for layer in self.layers:
            for A, B in layer.values():
                A[slot].zero_()
                B[slot].zero_()
        self.scaling[slot] = 0.0
