"""Tree-draft verification against the linear split-KV entry on the same (B, past, n), Llama-3-8B heads (32 / 8), in ONE run (HIP
events around the C entry, warm-up, median of the timed launches, every variant measured REPS times in alternation so that the spread
between repeated medians of the same thing is known; run it under `timeout`):

    B   past     n        the tree entry's only new cost is the mask of the one tile of new keys, so the figure is the RATIO
    1    8 192    8       qs_append_tree_attention / qs_append_attention_split (both with the planner's split count for
    1    8 192   32       max_past = past; the tree is a random forest, the linear entry sees the same rows as a chain) and the
    1    8 192   64       spread of the run.  KV4 and KV8.  Also the tree writer against the linear writer, and
    8    4 096   32       qs_kv_cache_commit_path alone (a random path of n / 2 nodes per sequence).

    python scripts/bench_append_tree.py [--iters 30] [--warmup 5] [--reps 3] > profiles/append_tree.txt
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scripts.bench_append_split import BASE, H, HKV, W, make_cache, median_us      # noqa: E402  (the same cache builder and timer)

SHAPES = [(1, 8192, 8), (1, 8192, 32), (1, 8192, 64), (8, 4096, 32)]


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
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    rng = np.random.default_rng(0)
    st = torch.cuda.current_stream().cuda_stream
    print(f"# {torch.cuda.get_device_name(0)}; Llama-3-8B heads H={H} Hkv={HKV}; us, median of {a.iters} launches, {a.reps} such medians per "
          f"variant in alternation: lowest .. highest (spread = highest - lowest)")
    summary = []
    for int4 in (True, False):
        for B, past, n in SHAPES:
            spt = HKV * (64 if int4 else 128)
            pools, tab, mb = make_cache(B, past, n, int4, dev, gen)
            raw = torch.randn((B * n, W), dtype=torch.float16, device=dev, generator=gen)
            cu_q = torch.arange(0, B + 1, device=dev, dtype=torch.int32) * n
            pl = torch.full((B,), past, dtype=torch.int32, device=dev)
            parents = [(-1 if i == 0 else int(rng.integers(0, i))) for _ in range(B) for i in range(n)]
            masks = A.tree_masks_from_parents(parents, cu_q).to(dev)
            # a random root-to-leaf-ish path of up to n / 2 nodes per sequence: follow first children from the root
            idx = np.zeros((B, n), np.int32)
            lens = np.zeros((B,), np.int32)
            for b in range(B):
                path, par = [0], parents[b * n:(b + 1) * n]
                while len(path) < max(1, n // 2):
                    kids = [c for c in range(path[-1] + 1, n) if par[c] == path[-1]]
                    if not kids:
                        break
                    path.append(kids[-1])
                idx[b, : len(path)], lens[b] = path, len(path)
            d_idx, d_lens = torch.from_numpy(idx).to(dev), torch.from_numpy(lens).to(dev)
            qkv_l, qkv_t = raw.clone(), raw.clone()
            out = torch.empty((B * n, H, 128), dtype=torch.float16, device=dev)
            tail = (B * n, B, n, mb, H, HKV, 128, W, H * 128, 64, spt, int(int4), 1)
            head = (out.data_ptr(), cu_q.data_ptr(), pl.data_ptr(), tab.data_ptr())
            wtail = (B * n, B, mb, H, HKV, 64, spt, 128, BASE, int(int4), 1, st)
            plan = append_attention_split_plan(B, n, past, H, HKV, int4)
            variants = {
                "linear writer": lambda: check(lib.qs_append_rope_update_kv_cache(qkv_l.data_ptr(), cu_q.data_ptr(), pl.data_ptr(),
                                                                                  tab.data_ptr(), *wtail), "bench"),
                "tree writer": lambda: check(lib.qs_append_tree_rope_update_kv_cache(qkv_t.data_ptr(), cu_q.data_ptr(), pl.data_ptr(),
                                                                                     tab.data_ptr(), masks.data_ptr(), *wtail), "bench"),
                f"linear split ({plan['splits']})": lambda: check(lib.qs_append_attention_split(qkv_l.data_ptr(), *head, *tail, past, 0, st), "bench"),
                f"tree ({plan['splits']})": lambda: check(lib.qs_append_tree_attention(qkv_t.data_ptr(), *head, masks.data_ptr(), *tail, past, 0, st),
                                                          "bench"),
                "linear un-split": lambda: check(lib.qs_append_attention_split(qkv_l.data_ptr(), *head, *tail, past, 1, st), "bench"),
                "tree un-split": lambda: check(lib.qs_append_tree_attention(qkv_t.data_ptr(), *head, masks.data_ptr(), *tail, past, 1, st), "bench"),
                f"commit_path (m={int(lens.min())}..{int(lens.max())})": lambda: check(lib.qs_kv_cache_commit_path(
                    tab.data_ptr(), pl.data_ptr(), d_idx.data_ptr(), d_lens.data_ptr(), B, n, mb, HKV, 64, spt, int(int4), 1, st), "bench"),
            }
            # (the writers rotate their buffers again on every launch: the values drift, the work does not; the attention
            #  variants are timed on whatever the buffers hold - finite rows after a few rotations of unit-norm pairs)
            for k in list(variants):                             # every variant once, checked, before anything is timed
                variants[k]()
                torch.cuda.synchronize()
            meds = {k: [] for k in variants}
            for _ in range(a.reps):
                for k, fn in variants.items():
                    meds[k].append(median_us(fn, a.iters, a.warmup))
            kv = "kv4" if int4 else "kv8"
            print(f"\nB={B} past={past} n={n} {kv}: plan {plan}")
            for k, v in meds.items():
                print(f"    {k:28s} {min(v):9.1f} .. {max(v):9.1f}   (spread {max(v) - min(v):6.1f})")
            for lin_k, tree_k, what in ((f"linear split ({plan['splits']})", f"tree ({plan['splits']})", "attention, planner's splits"),
                                        ("linear un-split", "tree un-split", "attention, un-split"), ("linear writer", "tree writer", "writer")):
                t_l, t_t = statistics.median(meds[lin_k]), statistics.median(meds[tree_k])
                spread = max(max(meds[x]) - min(meds[x]) for x in (lin_k, tree_k))
                verdict = "same within spread" if abs(t_t - t_l) <= spread else "slower" if t_t > t_l else "faster"
                summary.append(f"    B={B:<2d} past={past:<5d} n={n:<3d} {kv} {what:28s}: tree {t_t:8.1f} us, linear {t_l:8.1f} us, ratio {t_t / t_l:5.3f}, "
                               f"spread {spread:5.1f} us -> {verdict}")
            ck = [k for k in meds if k.startswith("commit_path")][0]
            summary.append(f"    B={B:<2d} past={past:<5d} n={n:<3d} {kv} {ck:28s}: {statistics.median(meds[ck]):8.1f} us")
            del pools, tab
    print("\n# summary: the tree entries against the linear ones (the ratio is the only new cost), and the path commit alone")
    print("\n".join(summary))


if __name__ == "__main__":
    main()
