"""What the page pool, admission and serve() cost, in ONE run (no pass / fail threshold; figures only), at the bench configuration:
Llama-3-8B shapes, KV4, synthetic weights, B = 64, prompt 1 024.  Method of scripts/bench_stop_update.py: medians of figures taken in
alternation, and the median of the pairwise differences.

  1. per captured step(): a pooled engine's step graph (one reserve launch at its head) and a static engine's - which launches exactly
     what the engine launched before the pool existed - from the same restored state.  Host clock around --replays replays + device
     synchronise, per-replay mean.
  2. the reserve launch alone on a pool of the engine's geometry (64 rows, 32 layers), device events around one launch: no row grows;
     every row grows by one page (the step that crosses a page boundary); 64 prompts of 1 024 tokens (16 pages each): 64 * 16 slots *
     32 layers * 2 = 65 536 eight-byte table stores and a binary search per slot from ONE workgroup of 256 threads - the table fill,
     to be read next to figure 1's step / 32, one layer's work.
  3. an admit() of 8 ragged prompts into the running batch: its wall time, which is also how long the 56 live rows stall (admission
     and decode do not share a pass), next to the step time.
  4. serve() over --requests requests with a long-tailed length mix: tokens / s, the peak of pages in use, and N against the static
     batch * mb.

Run it under `timeout`.

    python scripts/bench_page_pool.py [--replays 50] [--reps 9] [--requests 256] [--out profiles/page_pool.txt]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PROMPT, BATCH, MAX_NEW = 1024, 64, 640


def med(xs):
    return f"{statistics.median(xs):9.1f} ({min(xs):.1f} .. {max(xs):.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--requests", type=int, default=256)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    assert a.replays >= 10 and a.reps >= 3 and a.requests >= BATCH
    assert torch.cuda.is_available(), "bench_page_pool needs a GPU"
    from qserve_amd import paging
    from qserve_amd.decode import LLAMA3_8B, DecodeEngine
    dev = torch.device("cuda:0")
    cfg, lines = LLAMA3_8B, []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    static = DecodeEngine(cfg, batch=BATCH, prompt_len=PROMPT, max_new=MAX_NEW, device="cuda:0", seed=0)
    mb, L = static.mb, cfg["layers"]
    N = BATCH * mb                                             # the same memory as the static engine: figure 4 says how much serve() used
    say(f"# {torch.cuda.get_device_name(0)}; {cfg['name']} shapes, KV4, B = {BATCH}, prompt {PROMPT}, max_len {PROMPT + MAX_NEW}: mb = {mb}, "
        f"static pages batch * mb = {N}, pool N = {N}")
    pooled = DecodeEngine(cfg, batch=BATCH, prompt_len=PROMPT, max_new=MAX_NEW, device="cuda:0", seed=0, page_pool=N)
    prompt = torch.randint(0, cfg["vocab"], (BATCH * PROMPT,), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    saved = {}
    for name, eng in (("static", static), ("pooled", pooled)):
        eng.prefill_chunked(PROMPT, 256, prompt)
        eng.enable_drafting(prompt)
        saved[name] = (eng.tokens.clone(), eng.lengths.clone(), eng.history.clone(), eng.hidden.clone())
        eng.capture()

    def reset(name, eng):
        """tokens, lengths and the text as after the prefill; the pooled rows keep the pages they grew into (a reserve that has them
        grows nothing: the steady state of a step)."""
        for t, s in zip((eng.tokens, eng.lengths, eng.history, eng.hidden), saved[name]):
            t.copy_(s)
        eng._len_bound = PROMPT + 1

    def per_replay_us(name, eng, n):
        reset(name, eng)
        for _ in range(3):
            eng.graph.replay()
        reset(name, eng)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            eng.graph.replay()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / n

    say(f"\n# 1. host clock around {a.replays} replays of the captured step + device synchronise, us per replay; {a.reps} figures per graph in "
        "alternation (static = what the engine launched before the pool)")
    st, po = [], []
    for _ in range(a.reps):
        st.append(per_replay_us("static", static, a.replays))
        po.append(per_replay_us("pooled", pooled, a.replays))
    diffs = [y - x for x, y in zip(st, po)]
    say(f"    captured step   static {med(st)} us   pooled {med(po)} us   pooled - static: median of pairs {statistics.median(diffs):+7.2f} us "
        f"({min(diffs):+.2f} .. {max(diffs):+.2f});   one layer's share of the static step: {statistics.median(st) / L:.1f} us")
    pooled.check()

    say(f"\n# 2. the reserve launch alone, {BATCH} rows x {L} layers, mb = {mb}, N = {N}: device events around ONE launch, us; {a.reps} figures each")
    tables = [torch.zeros((BATCH, 2, mb), dtype=torch.int64, device=dev) for _ in range(L)]
    pools = [(torch.zeros((N + 1, 64), dtype=torch.uint8, device=dev), torch.zeros((N + 1, 64), dtype=torch.uint8, device=dev)) for _ in range(L)]
    pool = paging.PagePool(tables, pools, 64)                  # (64-byte pages: the launches never touch a page)
    ones = torch.ones((BATCH,), dtype=torch.int32, device=dev)
    full = torch.full((BATCH,), PROMPT + 1, dtype=torch.int32, device=dev)

    def launch_us(setup, lengths, extra):
        out = []
        for _ in range(a.reps + 1):
            setup()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            pool.reserve(lengths, extra)
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) * 1e3)
        return out[1:]                                         # (the first figure is the warm-up)

    def empty():
        pool.release(ones)

    def prompts_held():
        pool.release(ones)
        pool.reserve(ones, PROMPT)                             # slots 0 .. 1023: 16 pages per row

    say(f"    no row grows (lengths {PROMPT + 1}, extra 0 behind a held prompt)        {med(launch_us(prompts_held, full, 0))} us")
    say(f"    every row grows by one page (lengths {PROMPT + 1}, extra 1: slot 1024)   {med(launch_us(prompts_held, full, 1))} us")
    say(f"    the table fill: {BATCH} prompts of {PROMPT} tokens from an empty pool        {med(launch_us(empty, ones, PROMPT))} us   "
        f"[{BATCH * (PROMPT // 64) * L * 2} table stores from one workgroup]")
    pool.check(starved=True)

    say("\n# 3. admit() of 8 ragged prompts (64 .. 1 024 tokens, chunk 256) into rows 0 .. 7 of the running pooled batch: wall ms around the call + "
        f"device synchronise - also the stall of the 56 live rows; {a.reps} figures")
    g = torch.Generator().manual_seed(3)
    ragged = [torch.randint(0, cfg["vocab"], (n,), generator=g) for n in (64, 130, 257, 400, 512, 700, 900, 1024)]
    wall = []
    for _ in range(a.reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pooled.admit(range(8), ragged, chunk=256)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    say(f"    admit, {sum(p.numel() for p in ragged)} prompt tokens   {med(wall[1:])} ms   = {statistics.median(wall[1:]) * 1e3 / statistics.median(po):.1f} "
        "captured steps of the live rows")
    pooled.check()

    say(f"\n# 4. serve() over {a.requests} greedy requests, long-tailed mix (prompts 16 .. 1 024, new tokens 8 .. 512, mostly short), poll_every 8, chunk 256")
    lens = torch.clamp((torch.rand((a.requests,), generator=g) ** 3 * 1024).long(), min=16).tolist()
    news = torch.clamp((torch.rand((a.requests,), generator=g) ** 3 * 512).long(), min=8).tolist()
    reqs = [(torch.randint(0, cfg["vocab"], (p,), generator=g).tolist(), m) for p, m in zip(lens, news)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out, stats = pooled.serve(reqs, poll_every=8, chunk=256)
    dt = time.perf_counter() - t0
    made = sum(len(r["tokens"]) for r in out)
    say(f"    {made} tokens generated ({sum(lens)} prompt tokens) in {dt:.2f} s: {made / dt:.0f} tokens / s;   {stats}")
    say(f"    peak pages in use (at the read-backs) {stats['peak_pages']} of N = {N} = the static batch * mb")
    pooled.check()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
