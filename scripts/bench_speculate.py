"""The n-gram drafter and the closed speculative loop of DecodeEngine, in ONE run (no pass / fail threshold; figures only):

  1. the drafter launch alone (drafting.ngram_draft_tree): B = 64, history length L in {1 024, 8 192}, a 16-node and a 64-node tree, on a
     history of random tokens (vocabulary 32 000: almost every position is rejected by its first comparison) and on a repetitive one
     (a period of 97 tokens: every node finds long matches).  HIP events around --launches back-to-back launches, per-launch mean;
     --reps such figures per case in alternation: lowest .. highest.
  2. what the drafter adds to a captured round: one run_speculate() replay against one run_verify() replay of the same tree
     (Llama-3-8B shapes, KV4, synthetic weights, B = 8, prompt 1 024, 16 nodes), each from the same restored state, host clock around
     replay + device synchronise, median of --iters, --reps medians in alternation.
  3. accepted tokens per pass and tokens / s of --rounds run_speculate() replays against the same number of run() replays (captured
     decode steps), in two settings: free-running (the history is the random prompt plus what the synthetic model says - next to nothing
     repeats, so this is the cost side alone) and planted (the greedy continuation, taken from a twin engine's run() steps, is written
     into the history beforehand where only the drafter reads it - the best case: every pass accepts the tree's depth + 1 tokens
     while the continuation lasts).

Run it under `timeout`.

    python scripts/bench_speculate.py [--launches 50] [--iters 20] [--reps 3] [--rounds 16] [--out profiles/speculate_ngram.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PROMPT, B_ENGINE, B_DRAFT = 1024, 8, 64


def random_tree(rng, n):
    return [-1] + [int(rng.integers(0, i)) for i in range(1, n)]


def deep_tree(n, width=2):
    """A chain with `width` - 1 extra leaves per level: depth about n / width (what a drafter that expects acceptance would use)."""
    par, spine = [-1], 0
    while len(par) < n:
        first = len(par)
        for _ in range(width):
            if len(par) < n:
                par.append(spine)
        spine = first
    return par


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=16)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    assert a.launches >= 10 and a.iters >= 10 and a.reps >= 2 and a.rounds >= 4
    assert torch.cuda.is_available(), "bench_speculate needs a GPU"
    from qserve_amd import drafting
    from qserve_amd.decode import LLAMA3_8B, DecodeEngine, _tree_depths
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"# {torch.cuda.get_device_name(0)}; n-gram drafter (max_ngram 4, min_match 1; LDS capacity {drafting.LDS_TOKENS} tokens)")

    # ---- 1. the drafter launch ----------------------------------------------------------------------------------------------------
    say(f"\n# 1. ngram_draft_tree alone, B = {B_DRAFT}: HIP events around {a.launches} back-to-back launches, us per launch, {a.reps} figures per case "
        "in alternation: lowest .. highest")
    cases = {}
    for L in (1024, 8192):
        rand = rng.integers(0, 32000, size=(B_DRAFT, L)).astype(np.int32)
        rep = np.tile(rng.integers(0, 32000, size=(B_DRAFT, 97)), (1, L // 97 + 1))[:, :L].astype(np.int32)
        for n in (16, 64):
            par = torch.tensor(random_tree(rng, n), dtype=torch.int32, device=dev)
            for name, h in (("random", rand), ("periodic", rep)):
                hist = torch.from_numpy(h).to(dev)
                cases[(L, n, name)] = (hist, torch.full((B_DRAFT,), L, dtype=torch.int32, device=dev), par,
                                       torch.empty((B_DRAFT, n), dtype=torch.int64, device=dev))

    def launch_us(hist, lens, par, out):
        for _ in range(3):
            drafting.ngram_draft_tree(hist, lens, par, 4, 1, 0, out=out)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.launches):
            drafting.ngram_draft_tree(hist, lens, par, 4, 1, 0, out=out)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.launches

    figs = {k: [] for k in cases}
    for _ in range(a.reps):
        for k, args in cases.items():
            figs[k].append(launch_us(*args))
    for (L, n, name), v in figs.items():
        say(f"    L={L:<5d} n={n:<3d} {name:9s} {min(v):9.1f} .. {max(v):9.1f} us")
    del cases

    # ---- 2. and 3. the engine ---------------------------------------------------------------------------------------------------------
    max_new = 16 + 17 * (a.rounds + 8)
    prompt = torch.randint(0, LLAMA3_8B["vocab"], (B_ENGINE * PROMPT,), device=dev, generator=torch.Generator(device=dev).manual_seed(1))

    def engine():
        e = DecodeEngine(LLAMA3_8B, batch=B_ENGINE, prompt_len=PROMPT, max_new=max_new, device="cuda:0", seed=0)
        e.prefill_chunked(PROMPT, 256, prompt)
        e.enable_drafting(prompt)
        return e

    eng = engine()
    state0 = (eng.tokens.clone(), eng.lengths.clone(), eng.history.clone(), eng.hidden.clone())

    def reset(history=None):
        """tokens, lengths and the text as after the prefill (the cache behind the lengths is overwritten by whoever runs next)."""
        eng.tokens.copy_(state0[0])
        eng.lengths.copy_(state0[1])
        eng.history.copy_(state0[2] if history is None else history)
        eng.hidden.copy_(state0[3])
        eng._len_bound = PROMPT + 1

    par16 = deep_tree(16)
    depth = max(_tree_depths(par16))
    eng.capture_speculate(par16)
    reset()
    eng.capture_verify(par16)
    reset()
    eng.capture()
    reset()
    zero_draft = torch.zeros((B_ENGINE, 16), dtype=torch.int64, device=dev)

    def median_ms(fn):
        ts = []
        for i in range(3 + a.iters):
            reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts[3:])

    say(f"\n# 2. one captured round, {LLAMA3_8B['name']} shapes, KV4, B = {B_ENGINE}, prompt {PROMPT}, a 16-node tree of depth {depth}: host clock around "
        f"replay + device synchronise, ms, median of {a.iters}, {a.reps} medians in alternation: lowest .. highest")
    variants = {"run_verify (host-supplied draft)": lambda: eng.run_verify(zero_draft), "run_speculate (draft + verify + record)": eng.run_speculate}
    meds = {k: [] for k in variants}
    for _ in range(a.reps):
        for k, fn in variants.items():
            meds[k].append(median_ms(fn))
    for k, v in meds.items():
        say(f"    {k:42s} {min(v):8.3f} .. {max(v):8.3f} ms")
    t = {k: statistics.median(v) for k, v in meds.items()}
    ks = list(variants)
    say(f"    the drafter and the record add {t[ks[1]] - t[ks[0]]:+.3f} ms (median of medians; the largest spread of one variant is "
        f"{max(max(v) - min(v) for v in meds.values()):.3f} ms)")

    # the planted history: the greedy continuation of the prompt, from a twin's captured steps
    twin = engine()
    cont = [twin.tokens.clone()]
    twin.capture()                                               # (its warm-up is a real step)
    cont.append(twin.tokens.clone())
    for _ in range((depth + 1) * (a.rounds + 4)):
        twin.run()
        cont.append(twin.tokens.clone())
    del twin
    torch.cuda.empty_cache()
    cont = torch.stack(cont, dim=1).to(torch.int32)              # [B, 1 + M]: root, g1, g2, ...
    planted = state0[2].clone()
    planted[:, 16:16 + cont.size(1)] = cont                      # over prompt columns: only the drafter reads the history

    def rounds_per_s(fn, history):
        reset(history)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.rounds):
            fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        made = int((eng.lengths - state0[1]).sum())
        return made / (a.rounds * B_ENGINE), made / dt

    say(f"\n# 3. {a.rounds} replays from the state after the prefill: tokens per pass and sequence, tokens / s of the batch; {a.reps} figures each in "
        "alternation: lowest .. highest tokens / s")
    settings = {"run() (one token per pass)": (eng.run, None), "run_speculate, free-running": (eng.run_speculate, None),
                "run_speculate, planted continuation": (eng.run_speculate, planted)}
    res = {k: [] for k in settings}
    for _ in range(1 + a.reps):                                  # (the first pass over the settings is the warm-up)
        for k, (fn, h) in settings.items():
            res[k].append(rounds_per_s(fn, h))
    for k, v in res.items():
        v = v[1:]
        say(f"    {k:38s} {statistics.median(x[0] for x in v):6.2f} tokens / pass   {min(x[1] for x in v):10.1f} .. {max(x[1] for x in v):10.1f} tokens / s")
    say("    (synthetic weights: the free-running figure is the cost of a round that accepts next to nothing; the planted one is the best case of this "
        "tree, depth + 1 tokens per pass.  What a real model and real text accept lies between and is not measured here.)")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
