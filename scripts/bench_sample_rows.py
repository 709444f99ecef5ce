"""The row sampler (`qs_sample_rows`) against its two yardsticks, in ONE run, on logits of the Llama-3-8B vocabulary (n = 128 256):

    rows in {64, 64 * 16}  (a 64-sequence decode step; a 64-sequence verification of 16-node trees)
    x  greedy-equivalent (T = 1e-6)  |  T = 0.8  |  T = 0.8, k = 50, p = 0.9

    (a) `qs_argmax_rows` on the same buffer - the one-pass floor: it reads the same bytes once;
    (b) the torch path a sampler built from tensor ops takes: softmax(logits / T) (+ sort, cumsum and masks for top-k / top-p) and
        torch.multinomial.

HIP events around --iters back-to-back launches after warm-up launches of the same shape; the figure is the median of the per-launch
times of --reps such batches taken in alternation over the variants, so that the spread between repeated measurements of the same
thing is known.  No threshold: the file records times and ratios.  Run it under `timeout`.

    python scripts/bench_sample_rows.py [--iters 30] [--warmup 5] [--reps 3] [--out profiles/sample_rows.txt]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N = 128256
ROWS = (64, 64 * 16)
PARAMS = (("greedy-equivalent (T=1e-6)", 1e-6, 0, 1.0), ("T=0.8", 0.8, 0, 1.0), ("T=0.8 k=50 p=0.9", 0.8, 50, 0.9))


def torch_sampler(logits, T, k, p):
    """Temperature, top-p then top-k warpers and a multinomial draw with tensor ops (what the reference's sampler layer amounts to)."""
    if T < 1e-5:
        return torch.argmax(logits, dim=1)
    s = logits.float() / T
    if p < 1.0:
        srt, idx = torch.sort(s, dim=1, descending=True)
        pr = torch.softmax(srt, dim=1)
        drop = (torch.cumsum(pr, dim=1) - pr) >= p
        s = s.scatter(1, idx, srt.masked_fill(drop, float("-inf")))
    if 0 < k < s.size(1):
        kth = torch.topk(s, k, dim=1).values[:, -1:]
        s = s.masked_fill(s < kth, float("-inf"))
    return torch.multinomial(torch.softmax(s, dim=1), 1).squeeze(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    assert a.iters >= 10 and a.reps >= 2
    assert torch.cuda.is_available(), "bench_sample_rows needs a GPU"
    from qserve_amd.decode import argmax_rows_
    from qserve_amd.sampling import sample_rows
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def per_launch_us(fn):
        for _ in range(a.warmup):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.iters

    say(f"# {torch.cuda.get_device_name(0)}; fp16 logits [rows, {N}] (standard normal x 3); HIP events around {a.iters} back-to-back launches, "
        f"us per launch; {a.reps} such figures per variant in alternation: lowest .. highest")
    summary = []
    for rows in ROWS:
        logits = (torch.randn((rows, N), device=dev, generator=torch.Generator(device=dev).manual_seed(rows)) * 3.0).half()
        out = torch.empty((rows,), dtype=torch.int64, device=dev)
        keys = torch.arange(rows, dtype=torch.int64, device=dev)
        say(f"\nrows={rows}:")
        for name, T, k, p in PARAMS:
            variants = {
                "qs_sample_rows": lambda: sample_rows(logits, out, T, k, p, seed=1, row_keys=keys),
                "qs_argmax_rows": lambda: argmax_rows_(logits, out),
                "torch softmax + multinomial": lambda: torch_sampler(logits, T, k, p),
            }
            meds = {v: [] for v in variants}
            for _ in range(a.reps):
                for v, fn in variants.items():
                    meds[v].append(per_launch_us(fn))
            say(f"  {name}:")
            for v, t in meds.items():
                say(f"    {v:30s} {min(t):10.1f} .. {max(t):10.1f} us")
            t = {v: statistics.median(x) for v, x in meds.items()}
            summary.append(f"    rows={rows:<5d} {name:28s}: sample_rows {t['qs_sample_rows']:9.1f} us = x{t['qs_sample_rows'] / t['qs_argmax_rows']:6.2f} of "
                           f"argmax_rows ({t['qs_argmax_rows']:8.1f} us), x{t['qs_sample_rows'] / t['torch softmax + multinomial']:6.3f} of the torch path "
                           f"({t['torch softmax + multinomial']:9.1f} us)")
        del logits
        torch.cuda.empty_cache()
    say("\n# summary: medians, and qs_sample_rows as a multiple of each yardstick (below 1 = faster)")
    for s in summary:
        say(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
