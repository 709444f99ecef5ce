"""Append attention against its two yardsticks, Llama-3-8B heads (32 / 8), KV4, in ONE run (HIP events, warm-up, median of the
timed launches; run it under `timeout`):

  (a) chunked-prefill shape   B = 4, past 4096, n 512   vs  the prefill provider on fp16 k / v of the same lengths
                              (len_q 512, len_k 4608, causal)
  (b) verification shape      B = 64, past 1024, n 4    vs  the KV4 decode kernel at B = 64, L = 1028 (it streams the same cache
                              bytes); and the fraction of 8 TB/s on Hkv * past * (2 * 64 + 8) bytes per sequence

    python scripts/bench_append.py [--iters 30] [--warmup 5] > profiles/append_attention.txt
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H, HKV, BASE = 32, 8, 5e5
SPT = HKV * 64


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts), min(ts)


def make_cache(B, past, extra, dev, gen):
    """Pools + tables (scattered blocks) holding `past` tokens per sequence, written by the prefill writer."""
    from qserve_backend import fused_attention as fa
    mb = (past + extra + 63) // 64 + 1
    pb = HKV * 64 * 64 + 64 * HKV * 4
    nb = B * mb
    kp = torch.zeros((nb, pb), dtype=torch.uint8, device=dev)
    vp = torch.zeros((nb, pb), dtype=torch.uint8, device=dev)
    perm = torch.randperm(nb, generator=torch.Generator().manual_seed(1)).reshape(B, mb)
    t = torch.empty((B, 2, mb), dtype=torch.int64)
    t[:, 0] = kp.data_ptr() + perm * pb
    t[:, 1] = vp.data_ptr() + perm * pb
    t = t.to(dev)
    seq = torch.full((B,), past, dtype=torch.int32, device=dev)
    cu = torch.arange(0, B + 1, device=dev, dtype=torch.int32) * past
    pad = fa.compute_padding_offsets(cu, past, B * past)
    for b0 in range(0, B, 8):                                   # (in slices: the source rows are 12 KiB each)
        nbq = min(8, B - b0)
        src = torch.randn((nbq * past, (H + 2 * HKV) * 128), dtype=torch.float16, device=dev, generator=gen)
        fa.apply_bias_rope_update_kv_cache(src, seq[:nbq], pad[:nbq * past], t[b0:b0 + nbq].contiguous(), H, HKV, past, 64, SPT, 128,
                                           BASE, 8192, True, True, True)
    return (kp, vp), t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    assert a.iters >= 20
    from qserve_amd import append as A
    from qserve_amd.flash import flash_attn_varlen_func
    from qserve_amd.plan import append_attention_plan
    from qserve_backend import fused_attention as fa
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    print(f"# {torch.cuda.get_device_name(0)}; Llama-3-8B heads H={H} Hkv={HKV}, KV4; median (min) of {a.iters} launches, us")

    # ---- (a) chunked prefill ----------------------------------------------------------------------------------------------
    B, past, n = 4, 4096, 512
    pools, tab = make_cache(B, past, n, dev, gen)
    qkv = torch.randn((B * n, (H + 2 * HKV) * 128), dtype=torch.float16, device=dev, generator=gen)
    cu_q = torch.arange(0, B + 1, device=dev, dtype=torch.int32) * n
    pl = torch.full((B,), past, dtype=torch.int32, device=dev)
    A.append_rope_update_kv_cache(qkv, cu_q, pl, tab, H, HKV, SPT, BASE, True)
    out = torch.empty((B * n, H, 128), dtype=torch.float16, device=dev)
    t_app = timed(lambda: A.append_attention(qkv, cu_q, pl, tab, H, HKV, SPT, True, max_seqlen_q=n, out=out), a.iters, a.warmup)
    q = qkv[:, :H * 128].reshape(B * n, H, 128)
    k = torch.randn((B * (past + n), HKV, 128), dtype=torch.float16, device=dev, generator=gen)
    v = torch.randn((B * (past + n), HKV, 128), dtype=torch.float16, device=dev, generator=gen)
    cu_k = torch.arange(0, B + 1, device=dev, dtype=torch.int32) * (past + n)
    t_fl = timed(lambda: flash_attn_varlen_func(q, k, v, cu_q, cu_k, n, past + n, causal=True), a.iters, a.warmup)
    flops = 4.0 * B * H * 128 * (n * past + n * (n + 1) / 2)
    print(f"(a) B={B} past={past} n={n}  plan {append_attention_plan(B, n, H, HKV)}")
    print(f"    append_attention            {t_app[0]:9.1f} ({t_app[1]:9.1f})   {flops / t_app[0] * 1e-6:7.1f} TFLOP/s")
    print(f"    flash_attn_varlen (fp16 kv) {t_fl[0]:9.1f} ({t_fl[1]:9.1f})   {flops / t_fl[0] * 1e-6:7.1f} TFLOP/s")
    print(f"    ratio append / flash        {t_app[0] / t_fl[0]:9.3f}")
    del pools, tab, k, v

    # ---- (b) verification of drafted tokens -------------------------------------------------------------------------------
    B, past, n = 64, 1024, 4
    pools, tab = make_cache(B, past, 8, dev, gen)
    qkv = torch.randn((B * n, (H + 2 * HKV) * 128), dtype=torch.float16, device=dev, generator=gen)
    cu_q = torch.arange(0, B + 1, device=dev, dtype=torch.int32) * n
    pl = torch.full((B,), past, dtype=torch.int32, device=dev)
    A.append_rope_update_kv_cache(qkv, cu_q, pl, tab, H, HKV, SPT, BASE, True)
    out = torch.empty((B * n, H, 128), dtype=torch.float16, device=dev)
    t_app = timed(lambda: A.append_attention(qkv, cu_q, pl, tab, H, HKV, SPT, True, max_seqlen_q=n, out=out), a.iters, a.warmup)
    one = torch.randn((B, (H + 2 * HKV) * 128), dtype=torch.float16, device=dev, generator=gen)
    q1, k1, v1 = one.split([H * 128, HKV * 128, HKV * 128], dim=-1)
    lens = torch.full((B,), past + n, dtype=torch.int32, device=dev)          # L = 1028: the new token lands in slot 1027
    t_dec = timed(lambda: fa.single_query_attention(q1.reshape(B, H, 128), k1.reshape(B, HKV, 128), v1.reshape(B, HKV, 128), tab, lens,
                                                    None, 8192, 64, SPT, past + 8, 128, BASE, True, True, True), a.iters, a.warmup)
    cache_bytes = B * HKV * past * (2 * 64 + 8)
    print(f"(b) B={B} past={past} n={n}  plan {append_attention_plan(B, n, H, HKV)}")
    print(f"    append_attention            {t_app[0]:9.1f} ({t_app[1]:9.1f})   {cache_bytes / t_app[0] * 1e-6:6.2f} TB/s of cache bytes "
          f"= {cache_bytes / t_app[0] * 1e-6 / 8.0:5.3f} of 8 TB/s")
    print(f"    single_query_attention L={past + n} {t_dec[0]:7.1f} ({t_dec[1]:9.1f})   {cache_bytes / t_dec[0] * 1e-6:6.2f} TB/s")
    print(f"    ratio append / decode       {t_app[0] / t_dec[0]:9.3f}")


if __name__ == "__main__":
    main()
