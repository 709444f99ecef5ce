"""Split-KV append attention against the un-split entry, Llama-3-8B heads (32 / 8), in ONE run (HIP events around the C entry,
warm-up, median of the timed launches, every variant measured REPS times in alternation so that the spread between repeated medians
of the same thing is known; run it under `timeout`):

    B   past     n      B = 1 rows: the shapes the split exists for; B = 4 / 8 / 64: where the un-split grid already fills
    1    8 192    8     more of the chip.  KV4 everywhere, KV8 on the first row.
    1   32 768  512
    4    4 096  512     per shape: qs_append_attention, forced splits 2 .. 64 (where pages and the workspace allow), the planner's
    8    4 096    4     choice (num_splits = 0, max_past = past), and for n <= 8 the KV4 decode kernel at the same B and L (it
    64   1 024    4     streams the same cache bytes).  Two more rows (B = 1, past 1 024 / 2 048, n = 8) show the planner where the
                        minimum number of pages per split decides.

    python scripts/bench_append_split.py [--iters 30] [--warmup 5] [--reps 3] > profiles/append_split.txt
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H, HKV, BASE = 32, 8, 5e5
W = (H + 2 * HKV) * 128
SHAPES = [(1, 8192, 8, True), (1, 8192, 8, False), (1, 32768, 512, True), (4, 4096, 512, True), (8, 4096, 4, True), (64, 1024, 4, True),
          (1, 1024, 8, True), (1, 2048, 8, True)]      # the last two: short pasts, where the minimum of pages per split decides
FORCED = [2, 4, 8, 16, 32, 64]
WS_BYTES, WG_REC_BYTES = 32 << 20, 4 * 32 * 130 * 4     # the library's split-KV workspace; partial records of one workgroup


def median_us(fn, iters, warmup):
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
    return statistics.median(ts)


def make_cache(B, past, extra, int4, dev, gen):
    """Pools + tables (scattered blocks) holding `past` tokens per sequence, written by the prefill writer."""
    from qserve_backend import fused_attention as fa
    dhb = 64 if int4 else 128
    mb = (past + extra + 63) // 64 + 1
    pb = HKV * 64 * dhb + 64 * HKV * 4
    nb = B * mb
    kp = torch.zeros((nb, pb), dtype=torch.uint8, device=dev)
    vp = torch.zeros((nb, pb), dtype=torch.uint8, device=dev)
    perm = torch.randperm(nb, generator=torch.Generator().manual_seed(1)).reshape(B, mb)
    t = torch.empty((B, 2, mb), dtype=torch.int64)
    t[:, 0] = kp.data_ptr() + perm * pb
    t[:, 1] = vp.data_ptr() + perm * pb
    t = t.to(dev)
    per = max(1, 8192 // past)                                   # (in slices: the source rows are 12 KiB each)
    for b0 in range(0, B, per):
        nbq = min(per, B - b0)
        seq = torch.full((nbq,), past, dtype=torch.int32, device=dev)
        cu = torch.arange(0, nbq + 1, device=dev, dtype=torch.int32) * past
        pad = fa.compute_padding_offsets(cu, past, nbq * past)
        src = torch.randn((nbq * past, W), dtype=torch.float16, device=dev, generator=gen)
        fa.apply_bias_rope_update_kv_cache(src, seq, pad, t[b0:b0 + nbq].contiguous(), H, HKV, past, 64, HKV * dhb, 128, BASE,
                                           max(8192, past + extra), True, int4, True)
    return (kp, vp), t, mb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    assert a.iters >= 20 and a.reps >= 2
    from qserve_amd import append as A
    from qserve_amd._lib import check, lib
    from qserve_amd.plan import append_attention_split_plan
    from qserve_backend import fused_attention as fa
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    st = torch.cuda.current_stream().cuda_stream
    print(f"# {torch.cuda.get_device_name(0)}; Llama-3-8B heads H={H} Hkv={HKV}; us, median of {a.iters} launches, {a.reps} such medians per "
          f"variant in alternation: lowest .. highest (spread = highest - lowest)")
    summary = []
    for B, past, n, int4 in SHAPES:
        spt = HKV * (64 if int4 else 128)
        pools, tab, mb = make_cache(B, past, n, int4, dev, gen)
        qkv = torch.randn((B * n, W), dtype=torch.float16, device=dev, generator=gen)
        cu_q = torch.arange(0, B + 1, device=dev, dtype=torch.int32) * n
        pl = torch.full((B,), past, dtype=torch.int32, device=dev)
        A.append_rope_update_kv_cache(qkv, cu_q, pl, tab, H, HKV, spt, BASE, int4)
        out = torch.empty((B * n, H, 128), dtype=torch.float16, device=dev)
        args = (qkv.data_ptr(), out.data_ptr(), cu_q.data_ptr(), pl.data_ptr(), tab.data_ptr(), B * n, B, n, mb, H, HKV, 128, W, H * 128, 64,
                spt, int(int4), 1)
        plan = append_attention_split_plan(B, n, past, H, HKV, int4)
        pages = (past + 63) // 64
        cap = WS_BYTES // (B * HKV * plan["q_tiles"] * WG_REC_BYTES)
        variants = {"unsplit": lambda: check(lib.qs_append_attention(*args, st), "bench")}
        for s in FORCED:
            if s <= pages and s <= cap:
                variants[f"forced {s}"] = lambda s=s: check(lib.qs_append_attention_split(*args, past, s, st), "bench")
        variants[f"planner ({plan['splits']})"] = lambda: check(lib.qs_append_attention_split(*args, past, 0, st), "bench")
        if n <= 8 and int4:
            one = torch.randn((B, W), dtype=torch.float16, device=dev, generator=gen)
            q1, k1, v1 = (x.reshape(B, -1, 128) for x in one.split([H * 128, HKV * 128, HKV * 128], dim=-1))
            lens = torch.full((B,), past + n, dtype=torch.int32, device=dev)
            variants[f"decode kv4 L={past + n}"] = lambda: fa.single_query_attention(q1, k1, v1, tab, lens, None, max(8192, past + n), 64, spt,
                                                                                   past + n, 128, BASE, True, True, True)
        for k in list(variants):                                 # every variant once, checked, before anything is timed
            variants[k]()
            torch.cuda.synchronize()
        meds = {k: [] for k in variants}
        for _ in range(a.reps):
            for k, fn in variants.items():
                meds[k].append(median_us(fn, a.iters, a.warmup))
        # the split result against the un-split one, once per shape (the planner's choice; a sanity check, not the parity test)
        variants["unsplit"]()
        ref = out.clone()
        variants[f"planner ({plan['splits']})"]()
        torch.cuda.synchronize()
        diff = (out.float() - ref.float()).abs().max().item()
        print(f"\nB={B} past={past} n={n} {'kv4' if int4 else 'kv8'}: {B * HKV * plan['q_tiles']} un-split workgroups, {pages} pages, workspace "
              f"holds {cap} splits; plan {plan}; |planner - unsplit| max {diff:.2e}")
        un = meds["unsplit"]
        for k, v in meds.items():
            print(f"    {k:22s} {min(v):9.1f} .. {max(v):9.1f}   (spread {max(v) - min(v):6.1f})   x{statistics.median(v) / statistics.median(un):6.3f} of unsplit")
        pk = f"planner ({plan['splits']})"
        best = min((k for k in meds if k == "unsplit" or k.startswith("forced")), key=lambda k: statistics.median(meds[k]))
        spread = max(max(v) - min(v) for k, v in meds.items() if k == "unsplit" or k == pk)
        t_un, t_pl, t_best = statistics.median(un), statistics.median(meds[pk]), statistics.median(meds[best])
        summary.append((B, past, n, "kv4" if int4 else "kv8", plan["splits"], t_un, t_pl, spread, best, t_best))
        del pools, tab
    print("\n# summary: planner's choice against the un-split entry; regret = planner / best of (unsplit, forced counts)")
    for B, past, n, kv, s, t_un, t_pl, spread, best, t_best in summary:
        verdict = "faster" if t_un - t_pl > spread else "slower" if t_pl - t_un > spread else "same within spread"
        print(f"    B={B:<3d} past={past:<6d} n={n:<4d} {kv}: planner {s:2d} splits {t_pl:9.1f} us, unsplit {t_un:9.1f} us, spread {spread:6.1f} us "
              f"-> {verdict}; best {best} {t_best:9.1f} us, regret {t_pl / t_best:5.3f}")


if __name__ == "__main__":
    main()
