"""Decode attention for page tables of any length: `qs_single_query_attention_long` (csrc/attention_long.hip, include/qserve_amd.h).

`fused_attention.single_query_attention` sends pointer tables of more than 192 entries (12 288 tokens) to the VALU kernel, one workgroup
per sequence and KV head.  The entry here has the same contract - q and the new k rotated, the new token's K / V quantised into its page
slot, attention over the cached tokens plus the new one - on a split-KV matrix-core kernel whose page ranges are cut on the device from
`length_per_sample`, so a captured call stays valid while the lengths grow."""
import torch

from .backend._util import check, expect, guard, lib, ptr, stream


def page_ranges(length, splits, min_pages):
    """The cached-token ranges [(first, end)] a launch with `splits` ranges reads for a sequence of `length` tokens (the new one
    included): its n = ceil((length - 1) / 64) cached pages go evenly to r = clamp(n // min_pages, 1, splits) ranges, range z = pages
    [z n // r, (z + 1) n // r); the new token belongs to the last one.  (`plan.attention_long_plan` reports splits and min_pages.)"""
    past = length - 1
    n = (past + 63) // 64
    r = max(1, min(splits, n // min_pages))
    return [(z * n // r * 64, min((z + 1) * n // r * 64, past)) for z in range(r)]


def single_query_attention_long(q, k, v, kv_pointers, length_per_sample, size_per_token, timestep, rotary_base, int4_kv_cache=True,
                                memory_max_seqlen=8192, num_splits=0, window=0):
    """q [B, H, 128] / k, v [B, Hkv, 128] fp16 views of the qkv buffer (un-rotated new token), kv_pointers int64 [B, 2, max_blocks],
    length_per_sample int32 [B] (the new token included) or None (every sequence has `timestep` cached tokens) -> fp16 [B, H, 128].
    rotary_base: a base or a registered profile's key (qserve_amd/rope.py).  num_splits: 0 = the planner's count for the table, >= 1 = that
    many page ranges per sequence and KV head (cut to 64 and to the split-KV workspace).
    window: 0 = none; W >= 1 = sliding-window attention through `qs_single_query_attention_window` (csrc/attention_window.hip): the new
    token at position p sees key j iff p - W < j <= p - the last W - 1 cached tokens and itself -, the page ranges are cut from the
    window's pages, and the new token's K / V are written as without a window."""
    if int(window) < 0:
        raise RuntimeError(f"long_decode.single_query_attention_long: window={window} (0 = none, >= 1 = a sliding window of that many keys)")
    for n, t in (("q", q), ("k", k), ("v", v)):
        expect(t, torch.float16, n, contiguous=False)
    expect(kv_pointers, torch.int64, "kv_pointers")
    batch, nheads, nheads_kv, headdim = kv_pointers.size(0), q.size(1), k.size(1), k.size(-1)
    for n, t in (("q", q), ("k", k), ("v", v)):
        if not (t.stride(2) == 1 and t.stride(1) == headdim):
            raise RuntimeError(f"{n} must have stride(2) == 1 and stride(1) == head_dim")
    if k.stride(0) != v.stride(0):
        raise RuntimeError("k and v must have the same token stride (views of one qkv buffer, or equally padded buffers)")
    if length_per_sample is not None:
        expect(length_per_sample, torch.int32, "length_per_sample")
        if tuple(length_per_sample.shape) != (batch,):
            raise RuntimeError("length_per_sample must have shape (batch_size)")
    out = torch.empty((q.size(0), nheads, headdim), dtype=q.dtype, device=q.device)
    args = (ptr(q), ptr(k), ptr(v), ptr(kv_pointers), ptr(length_per_sample), ptr(out), batch, nheads, nheads_kv, headdim, q.stride(0),
            k.stride(0), kv_pointers.size(-1), int(memory_max_seqlen), 64, int(size_per_token), int(timestep), 128, float(rotary_base), 1,
            int(bool(int4_kv_cache)), 1)
    with guard(q):
        if int(window) > 0:
            check(lib.qs_single_query_attention_window(*args, int(window), int(num_splits), stream()),
                  "long_decode.single_query_attention_long")
        else:
            check(lib.qs_single_query_attention_long(*args, int(num_splits), stream()), "long_decode.single_query_attention_long")
    return out
