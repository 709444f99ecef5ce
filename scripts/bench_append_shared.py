"""Shared-prefix append attention against the split-KV entry on the SAME aliased tables, Llama-3-8B heads (32 / 8), in ONE run (HIP
events around the C entries, warm-up, median of the timed launches, every variant measured REPS times in alternation so that the
spread between repeated medians of the same thing is known; run it under `timeout`):

    B (one group unless noted)   prefix   own past   n     cache
    64                            1 024       64      1    KV4
    64                            1 024       64      4    KV4, KV8
    64                            4 096      128      4    KV4
    16                            8 192      512      8    KV4, KV8
    8 in two groups of 4          4 096      256     32    KV4
    8                             4 096        0    512    KV4      chunked prefill: compute-bound, expected roughly equal
    64 groups of 1                1 024        -      4    KV4      the planner declines (P = 0): must equal the baseline

per row: qs_append_attention_split with its planner (the baseline), qs_append_attention_shared with the planner's (P, S), and forced
P in {1, 2, 4, 8, 16, 32} (where the prefix has that many pages) with S from the planner.  A forced P the workspace cannot hold is
cut by the entry (down to 0 = the split entry's launch); the effective count is what qs_append_shared_plan's rule gives, printed
as "P -> effective".  Then, per candidate of the prefix role's minimum pages per split, the P the rule would choose and its regret
against the best measured forced count - the table MIN_PAGES_PREFIX in qserve_amd/csrc/append_shared.hip is fixed with.

    python scripts/bench_append_shared.py [--iters 30] [--warmup 5] [--reps 3] > profiles/append_shared.txt
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H, HKV, BASE = 32, 8, 5e5
W = (H + 2 * HKV) * 128
# (group sizes, prefix, own past, n, int4)
ROWS = [((64,), 1024, 64, 1, True), ((64,), 1024, 64, 4, True), ((64,), 1024, 64, 4, False), ((64,), 4096, 128, 4, True),
        ((16,), 8192, 512, 8, True), ((16,), 8192, 512, 8, False), ((4, 4), 4096, 256, 32, True), ((8,), 4096, 0, 512, True),
        ((1,) * 64, 1024, 0, 4, True)]
FORCED = [1, 2, 4, 8, 16, 32]
MIN_PAGES = [1, 2, 4, 8]
FILL, WS_BYTES, REC = 512, 32 << 20, 32 * 130 * 4


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


def make_cache(sizes, prefix, past, extra, int4, dev, gen):
    """Pools + tables (scattered blocks) holding `past` tokens per sequence, written by the prefill writer; then the members' entries
    below prefix / 64 point at their group's first member's pages."""
    from qserve_backend import fused_attention as fa
    B = sum(sizes)
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
    f = 0
    for n in sizes:
        t[f:f + n, :, :prefix // 64] = t[f:f + 1, :, :prefix // 64]
        f += n
    return (kp, vp), t, mb


def rule_P(min_pages, groups, gq_tiles, B, q_tiles, prefix, own, per_p, per_s):
    """qs_append_shared_plan's rule for the prefix role with another minimum of pages per split (the header of append_shared.hip)."""
    pages_p, pages_s = prefix // 64, (own + 63) // 64
    tiles = groups * gq_tiles * HKV * pages_p + B * q_tiles * HKV * (pages_s + 1)
    P = max(1, min(pages_p * FILL // tiles, pages_p // min_pages, 64))
    return max(0, min(P, (WS_BYTES - per_s) // per_p)) if per_s <= WS_BYTES else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    assert a.iters >= 20 and a.reps >= 2
    from qserve_amd import append as A
    from qserve_amd._lib import check, lib
    from qserve_amd.plan import append_attention_split_plan, append_shared_plan
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    st = torch.cuda.current_stream().cuda_stream
    print(f"# {torch.cuda.get_device_name(0)}; Llama-3-8B heads H={H} Hkv={HKV}; us, median of {a.iters} launches, {a.reps} such medians per "
          f"variant in alternation: lowest .. highest (spread = highest - lowest)")
    summary, regrets = [], {m: [] for m in MIN_PAGES}
    for sizes, prefix, own, n, int4 in ROWS:
        B, past, spt = sum(sizes), prefix + own, HKV * (64 if int4 else 128)
        pools, tab, mb = make_cache(sizes, prefix, past, n, int4, dev, gen)
        qkv = torch.randn((B * n, W), dtype=torch.float16, device=dev, generator=gen)
        cu_q = torch.arange(0, B + 1, device=dev, dtype=torch.int32) * n
        pl = torch.full((B,), past, dtype=torch.int32, device=dev)
        A.append_rope_update_kv_cache(qkv, cu_q, pl, tab, H, HKV, spt, BASE, int4)
        go, pf, sg = A.shared_prefix_groups(sizes, [prefix] * len(sizes), dev, batch=B)
        out = torch.empty((B * n, H, 128), dtype=torch.float16, device=dev)
        mgt = max(sizes) * n
        head = (qkv.data_ptr(), out.data_ptr(), cu_q.data_ptr(), pl.data_ptr(), tab.data_ptr())
        tail = (mb, H, HKV, 128, W, H * 128, 64, spt, int(int4), 1)
        split = lambda: check(lib.qs_append_attention_split(*head, B * n, B, n, *tail, past, 0, st), "bench")                 # noqa: E731
        shared = lambda P: check(lib.qs_append_attention_shared(*head, go.data_ptr(), pf.data_ptr(), sg.data_ptr(), B * n, B, len(sizes), n,  # noqa: E731
                                                                mgt, *tail, prefix, own, P, 0, st), "bench")
        plan = append_shared_plan(B, n, len(sizes), mgt, prefix, own, H, HKV, int4)
        base_plan = append_attention_split_plan(B, n, past, H, HKV, int4)
        per_p = len(sizes) * plan["group_q_tiles"] * HKV * max(plan["rec_waves_prefix"], min(4, -(-min(32, mgt) * 4 // 32))) * REC
        per_s = B * plan["q_tiles"] * HKV * min(4, -(-min(32, n) * 4 // 32)) * REC
        eff = lambda P: max(0, min(P, (WS_BYTES - per_s) // per_p)) if per_s <= WS_BYTES else 0      # noqa: E731  (what the entry runs)
        variants = {"split (baseline)": split, "shared planner": lambda: shared(0)}
        for P in FORCED:
            if P <= prefix // 64 and len(sizes) < B:
                variants[f"shared P={P} -> {eff(P)}"] = lambda P=P: shared(P)
        for k in list(variants):                                 # every variant once, checked, before anything is timed
            variants[k]()
            torch.cuda.synchronize()
        meds = {k: [] for k in variants}
        for _ in range(a.reps):
            for k, fn in variants.items():
                meds[k].append(median_us(fn, a.iters, a.warmup))
        split()
        ref = out.clone()
        shared(0)
        torch.cuda.synchronize()
        diff = (out.float() - ref.float()).abs().max().item()    # (a sanity check, not the parity test)
        print(f"\ngroups={sizes if len(sizes) < 5 else str(len(sizes)) + ' x 1'} prefix={prefix} own={own} n={n} {'kv4' if int4 else 'kv8'}: "
              f"baseline plan {base_plan['splits']} splits; shared plan P={plan['prefix_splits']} S={plan['suffix_splits']} "
              f"rec_waves {plan['rec_waves_prefix']}/{plan['rec_waves_suffix']} workspace {plan['workspace_bytes'] >> 10} KiB; "
              f"|shared - split| max {diff:.2e}")
        med = {k: statistics.median(v) for k, v in meds.items()}
        for k, v in meds.items():
            print(f"    {k:24s} {min(v):9.1f} .. {max(v):9.1f}   (spread {max(v) - min(v):6.1f})   x{med[k] / med['split (baseline)']:6.3f} of baseline")
        forced = {int(k.split("=")[1].split()[0]): med[k] for k in med if k.startswith("shared P=") and eff(int(k.split("=")[1].split()[0])) > 0}
        t_b, t_p = med["split (baseline)"], med["shared planner"]
        spread = max(max(meds[k]) - min(meds[k]) for k in ("split (baseline)", "shared planner"))
        best = min(forced, key=forced.get) if forced else None
        summary.append((sizes, prefix, own, n, "kv4" if int4 else "kv8", plan["prefix_splits"], plan["suffix_splits"], t_b, t_p, spread, best,
                        forced.get(best)))
        if forced and plan["prefix_splits"] > 0:
            for m in MIN_PAGES:                                  # the rule with another minimum: its P, timed as the nearest measured count below it
                P = rule_P(m, len(sizes), plan["group_q_tiles"], B, plan["q_tiles"], prefix, own, per_p, per_s)
                near = max((f for f in forced if f <= max(P, 1)), default=min(forced))
                regrets[m].append((P, near, forced[near] / forced[best]))
        del pools, tab
    print("\n# summary: the shared entry with the planner's (P, S) against the split entry with its planner; regret = planner / best forced P")
    for sizes, prefix, own, n, kv, P, S, t_b, t_p, spread, best, t_best in summary:
        verdict = "faster" if t_b - t_p > spread else "slower" if t_p - t_b > spread else "same within spread"
        tailtxt = f"best forced P={best} {t_best:9.1f} us, regret {t_p / t_best:5.3f}" if best and P > 0 else "planner declines (the split entry's launch)"
        print(f"    groups={str(sizes) if len(sizes) < 5 else str(len(sizes)) + ' x 1':8s} prefix={prefix:<5d} own={own:<4d} n={n:<4d} {kv}: baseline "
              f"{t_b:9.1f} us, shared (P={P}, S={S}) {t_p:9.1f} us, spread {spread:6.1f} us, x{t_p / t_b:5.3f} -> {verdict}; {tailtxt}")
    print("\n# prefix role, minimum pages per split: per row (P by the rule, nearest measured count <= it, its time / best forced), worst regret")
    for m in MIN_PAGES:
        r = regrets[m]
        print(f"    min pages {m}: " + "  ".join(f"({P},{near},{x:5.3f})" for P, near, x in r) + f"   worst {max(x for _, _, x in r):5.3f}")


if __name__ == "__main__":
    main()
