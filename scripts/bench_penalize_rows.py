"""The penalty launch (`qs_penalize_rows`) against its two yardsticks, in ONE run, on logits of the Llama-3-8B vocabulary (n = 128 256):

    B in {1, 64}  x  n_nodes in {1, 16, 64}  x  history of {1 024, 8 192} tokens per sequence
    (n_nodes = 1: a decode step; 16 / 64: a verification of the heap-shaped tree parents[i] = (i - 1) // 2)

    (a) the torch path a penalty built from tensor ops takes: scatter-add of the context into dense [rows, n] counts (all tokens, and
        generated tokens), then the elementwise rule over the whole row; its index tensors are built outside the timed region;
    (b) `qs_sample_rows` (T = 0.8, k = 50, p = 0.9) on the same rows - the launch the penalty sits in front of.

Histories are uniform random ids with every fourth token a repeat of an earlier one; the first half counts as prompt.  HIP events around
--iters back-to-back launches after warm-up launches of the same shape give one figure: the batch's time divided by --iters, a MEAN per
launch.  --reps such figures per variant are taken in alternation over the variants, so that the spread between repeated measurements of
the same thing is known; the report prints their lowest and highest and, in the summary, their median (of three by default).  (The
launches edit the same rows again and again: the values drift, the work per launch does not.)  No threshold: the file records times and
ratios.  Run it under `timeout`.

    python scripts/bench_penalize_rows.py [--iters 30] [--warmup 5] [--reps 3] [--out profiles/penalize_rows.txt]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N = 128256
BATCHES = (1, 64)
NODES = (1, 16, 64)
HISTORIES = (1024, 8192)
REP, FREQ, PRES = 1.1, 0.01, 0.01


def heap_tree(n):
    return [-1] + [(i - 1) // 2 for i in range(1, n)]


def path_table(par):
    """[n, depth] node indices of the nodes != 0 on the path root -> i, padded with -1."""
    paths = []
    for i in range(len(par)):
        p, j = [], i
        while j > 0:
            p.append(j)
            j = par[j]
        paths.append(p[::-1])
    width = max(1, max(len(p) for p in paths))
    return [p + [-1] * (width - len(p)) for p in paths]


def torch_context(history, lengths, prompt_lens, nodes, par):
    """(ids int64 [rows, C], weight of every entry towards c_all, towards c_gen) for the torch path: history, then the path, padded
    entries with weight 0."""
    B, cap = history.shape
    n = len(par)
    pos = torch.arange(cap, device=history.device)
    live = (pos.view(1, -1) < lengths.view(-1, 1)).float()
    gen = live * (pos.view(1, -1) >= prompt_lens.view(-1, 1)).float()
    ids = history.long().view(B, 1, cap).expand(B, n, cap)
    w_all, w_gen = live.view(B, 1, cap).expand(B, n, cap), gen.view(B, 1, cap).expand(B, n, cap)
    if n > 1:
        table = torch.tensor(path_table(par), device=history.device)                      # [n, D]
        on = (table >= 0).float().view(1, n, -1).expand(B, n, -1)
        pid = torch.gather(nodes.view(B, 1, n).expand(B, n, n), 2, table.clamp(min=0).view(1, n, -1).expand(B, n, -1))
        ids, w_all, w_gen = torch.cat([ids, pid], 2), torch.cat([w_all, on], 2), torch.cat([w_gen, on], 2)
    rows = B * n
    return ids.reshape(rows, -1).contiguous(), w_all.reshape(rows, -1).contiguous(), w_gen.reshape(rows, -1).contiguous()


def torch_penalize(logits, ids, w_all, w_gen):
    c_all = torch.zeros(logits.shape, dtype=torch.float32, device=logits.device).scatter_add_(1, ids, w_all)
    c_gen = torch.zeros(logits.shape, dtype=torch.float32, device=logits.device).scatter_add_(1, ids, w_gen)
    x = logits.float()
    y = torch.where(x > 0, x / REP, x * REP) - (FREQ * c_gen + PRES * (c_gen > 0))
    logits.copy_(torch.where(c_all > 0, y, x))
    return logits


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    assert a.iters >= 10 and a.reps >= 2
    assert torch.cuda.is_available(), "bench_penalize_rows needs a GPU"
    from qserve_amd.penalties import penalize_rows
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

    say(f"# {torch.cuda.get_device_name(0)}; fp16 logits [B * n_nodes, {N}] (standard normal x 3); repetition {REP}, frequency {FREQ}, presence "
        f"{PRES}; HIP events around {a.iters} back-to-back launches, mean us per launch; {a.reps} such figures per variant in alternation: "
        f"lowest .. highest")
    summary = []
    for B in BATCHES:
        for n in NODES:
            rows = B * n
            gen = torch.Generator(device=dev).manual_seed(rows)
            logits = (torch.randn((rows, N), device=dev, generator=gen) * 3.0).half()
            out = torch.empty((rows,), dtype=torch.int64, device=dev)
            keys = torch.arange(rows, dtype=torch.int64, device=dev)
            par = heap_tree(n)
            tree = torch.tensor(par, dtype=torch.int32, device=dev)
            for L in HISTORIES:
                history = torch.randint(0, N, (B, L), device=dev, generator=gen).int()
                history[:, 3::4] = history[:, 1:L - 2:4]                                   # every fourth token repeats an earlier one
                lengths = torch.full((B,), L, dtype=torch.int32, device=dev)
                prompt_lens = torch.full((B,), L // 2, dtype=torch.int32, device=dev)
                nodes = torch.randint(0, N, (B, n), device=dev, generator=gen)
                nodes[:, 1:] = history[:, 5:5 + n - 1]                                     # a draft repeats the text
                ids, w_all, w_gen = torch_context(history, lengths, prompt_lens, nodes, par)
                variants = {
                    "qs_penalize_rows": lambda: penalize_rows(logits, history, lengths, prompt_lens, nodes if n > 1 else None,
                                                              tree if n > 1 else None, REP, FREQ, PRES),
                    "torch scatter_add + where": lambda: torch_penalize(logits, ids, w_all, w_gen),
                    "qs_sample_rows": lambda: sample_rows(logits, out, 0.8, 50, 0.9, seed=1, row_keys=keys),
                }
                meds = {v: [] for v in variants}
                for _ in range(a.reps):
                    for v, fn in variants.items():
                        meds[v].append(per_launch_us(fn))
                say(f"\nB={B} n_nodes={n} history={L} ({rows} rows):")
                for v, t in meds.items():
                    say(f"    {v:28s} {min(t):10.1f} .. {max(t):10.1f} us")
                t = {v: statistics.median(x) for v, x in meds.items()}
                summary.append(f"    B={B:<3d} n_nodes={n:<3d} history={L:<5d}: penalize_rows {t['qs_penalize_rows']:9.1f} us = "
                               f"x{t['qs_penalize_rows'] / t['torch scatter_add + where']:7.4f} of the torch path "
                               f"({t['torch scatter_add + where']:10.1f} us), x{t['qs_penalize_rows'] / t['qs_sample_rows']:6.3f} of sample_rows "
                               f"({t['qs_sample_rows']:9.1f} us)")
                del ids, w_all, w_gen
            del logits
            torch.cuda.empty_cache()
    say(f"\n# summary: the median of the {a.reps} figures of each variant, and qs_penalize_rows as a multiple of each yardstick (below 1 = faster)")
    for s in summary:
        say(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
