"""Row sampler (extension; NOT part of the reference's `qserve_backend` surface - its sampler layer is torch ops): one token per row of
fp16 logits under temperature, top-k and top-p, on the device, reproducible and capturable in a hipGraph.

    sample_rows      the draw; include/qserve_amd.h (`qs_sample_rows`) has the contract - thresholds are logit VALUES (a tie class stays
                     whole), the nucleus is cut on the full tempered distribution and then intersected with top-k, the cumulative sum of
                     the draw runs in index order
    position_keys    the Philox keys that make sampled decoding independent of what was drafted: one key per (sequence, position)

The uniform of a row is a function of (seed, key) alone: the kernel has no state, so a replayed graph draws new numbers exactly when the
keys change on the device.  Backed by qserve_amd/csrc/sample_rows.hip."""
import torch

from .backend._util import check, expect, guard, lib, ptr, stream


def _row_param(v, dtype, rows, name, device, what):
    """A scalar -> (scalar, None); a device tensor [rows] -> (neutral scalar, tensor)."""
    if isinstance(v, torch.Tensor):
        expect(v, dtype, name)
        if tuple(v.shape) != (rows,) or v.device != device:
            raise RuntimeError(f"{what}: {name} must be a scalar or a [{rows}] tensor on {device}, got {tuple(v.shape)} on {v.device}")
        return None, v
    return v, None


def sample_rows(logits, out=None, temperature=1.0, top_k=0, top_p=1.0, uniforms=None, seed=0, row_keys=None, u_out=None):
    """out[r] = a token drawn from softmax(logits[r] / temperature) restricted by top-k and top-p (fp16 [rows, n] -> int64 [rows]).
    `temperature`, `top_k`, `top_p`: a scalar each, or a device tensor [rows] (float32, int32, float32) for per-row values.  temperature
    < 1e-5 or top_p < 1e-8 is greedy (the first maximum); top_k <= 0 or >= n and top_p >= 1 switch the filter off.  The row's uniform is
    `uniforms[r]` (float32 [rows], in [0, 1)) when given, else the Philox4x32-10 draw of (`seed`, key) with key = `row_keys[r]` (int64
    [rows]) or r; `u_out` (float32 [rows]) receives the uniform every row used.  Rows need n >= 8, a unit column stride and a row stride
    that is a multiple of 8.  -> out."""
    what = "sampling.sample_rows"
    expect(logits, torch.float16, "logits", contiguous=False)
    if logits.dim() != 2 or logits.stride(1) != 1:
        raise RuntimeError(f"{what}: logits must be [rows, n] with a unit column stride, got {tuple(logits.shape)}, strides {logits.stride()}")
    rows, n = logits.shape
    if n < 8 or logits.stride(0) < n or logits.stride(0) % 8 != 0:
        raise RuntimeError(f"{what}: n={n} must be >= 8 and the row stride {logits.stride(0)} a multiple of 8 that is >= n")
    dev = logits.device
    if out is None:
        out = torch.empty((rows,), dtype=torch.int64, device=dev)
    for t, dt, name in ((out, torch.int64, "out"), (uniforms, torch.float32, "uniforms"), (row_keys, torch.int64, "row_keys"),
                        (u_out, torch.float32, "u_out")):
        if t is None:
            continue
        expect(t, dt, name)
        if t.dim() != 1 or t.numel() < rows or t.device != dev:
            raise RuntimeError(f"{what}: {name} must be a 1-d tensor of at least {rows} entries on {dev}, got {tuple(t.shape)} on {t.device}")
    temperature, row_t = _row_param(temperature, torch.float32, rows, "temperature", dev, what)
    top_k, row_k = _row_param(top_k, torch.int32, rows, "top_k", dev, what)
    top_p, row_p = _row_param(top_p, torch.float32, rows, "top_p", dev, what)
    seed = int(seed)
    if not 0 <= seed < 1 << 64:
        raise RuntimeError(f"{what}: seed={seed} must fit 64 unsigned bits")
    if rows == 0:                      # (an empty tensor has no address to hand over)
        return out
    with guard(logits):
        check(lib.qs_sample_rows(ptr(logits), ptr(out), rows, n, logits.stride(0), 1.0 if row_t is not None else float(temperature),
                                 0 if row_k is not None else int(top_k), 1.0 if row_p is not None else float(top_p), ptr(row_t), ptr(row_k),
                                 ptr(row_p), ptr(uniforms), seed, ptr(row_keys), ptr(u_out), stream()), what)
    return out


def position_keys(seq_ids, positions):
    """int64 seq << 32 | position, elementwise (device ops only): the key of the token at `positions` of sequence `seq_ids`."""
    return (seq_ids.to(torch.int64) << 32) | (positions.to(torch.int64) & 0xFFFFFFFF)
