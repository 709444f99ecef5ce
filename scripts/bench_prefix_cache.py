"""What reference counts and the prefix cache cost and save, in ONE run (no pass / fail threshold; figures only), at the bench
configuration: Llama-3-8B shapes, KV4, synthetic weights, B = 64, prompt 1 024.  Method of scripts/bench_page_pool.py: medians of
figures taken in alternation, and the median of the pairwise differences.  The hit rate stands beside every figure that has one.

  1. the allocator launches alone on a pool of the engine's geometry (64 rows, 32 layers), device events around ONE launch: the counted
     reserve beside the uncounted one re-measured in the same run (no row grows; 64 rows grow by a page; 64 prompts of 1 024 tokens),
     a hold of 15 pages into each of 64 rows, and the unhold of those rows beside the uncounted release.
  2. per captured step(): a counted pooled engine's step graph beside an uncounted pooled engine's, from the same restored state, in
     interleaved pairs.  Host clock around --replays replays + device synchronise, per-replay mean.
  3. an admit() of 8 prompts of 1 024 tokens whose first 960 are cached, beside the same admit on the uncounted engine.
  4. serve() over --requests requests behind a common prefix of 1 024 tokens (own tails 16 .. 256, 8 .. 128 new tokens), with and
     without the cache: tokens / s, peak pages, preemptions.

Run it under `timeout`.

    python scripts/bench_prefix_cache.py [--replays 50] [--reps 9] [--requests 256] [--out profiles/prefix_cache.txt]
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
    assert torch.cuda.is_available(), "bench_prefix_cache needs a GPU"
    from qserve_amd import paging
    from qserve_amd.decode import LLAMA3_8B, DecodeEngine
    dev = torch.device("cuda:0")
    cfg, lines = LLAMA3_8B, []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    L = cfg["layers"]
    mb = (PROMPT + MAX_NEW + 63) // 64 + 1
    N = BATCH * mb
    say(f"# {torch.cuda.get_device_name(0)}; {cfg['name']} shapes, KV4, B = {BATCH}, prompt {PROMPT}, max_len {PROMPT + MAX_NEW}: mb = {mb}, pool N = {N}")

    # ---- 1. the launches alone
    say(f"\n# 1. the allocator launches alone, {BATCH} rows x {L} layers, mb = {mb}, N = {N}: device events around ONE launch, us; {a.reps} figures "
        "each, counted and uncounted in alternation")
    pools_ = {}
    for counted in (False, True):
        tables = [torch.zeros((BATCH, 2, mb), dtype=torch.int64, device=dev) for _ in range(L)]
        pools = [(torch.zeros((N + 1, 64), dtype=torch.uint8, device=dev), torch.zeros((N + 1, 64), dtype=torch.uint8, device=dev)) for _ in range(L)]
        pools_[counted] = paging.PagePool(tables, pools, 64, refcounts=counted)       # (64-byte pages: the launches never touch a page)
    ones = torch.ones((BATCH,), dtype=torch.int32, device=dev)
    full = torch.full((BATCH,), PROMPT + 1, dtype=torch.int32, device=dev)

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3

    def both(setup, launch):
        out = {False: [], True: []}
        for _ in range(a.reps + 1):
            for counted in (False, True):
                setup(pools_[counted])
                out[counted].append(timed(lambda: launch(pools_[counted])))
        return f"uncounted {med(out[False][1:])} us   counted {med(out[True][1:])} us"

    def empty(pool):
        pool.release(ones)

    def prompts_held(pool):
        pool.release(ones)
        pool.reserve(ones, PROMPT)

    say(f"    reserve, no row grows (lengths {PROMPT + 1}, extra 0)              {both(prompts_held, lambda p: p.reserve(full, 0))}")
    say(f"    reserve, every row grows by one page (extra 1: slot 1024)   {both(prompts_held, lambda p: p.reserve(full, 1))}")
    say(f"    reserve, {BATCH} prompts of {PROMPT} tokens from an empty pool          {both(empty, lambda p: p.reserve(ones, PROMPT))}")
    say(f"    release / unhold of {BATCH} rows of 16 pages                       {both(prompts_held, lambda p: p.release(ones))}")
    pool = pools_[True]
    take = torch.where(torch.arange(BATCH, device=dev) == 0, 0, 15).to(torch.int32)
    hold, unhold = [], []
    from qserve_amd._lib import lib
    from qserve_amd.backend._util import check, ptr, stream
    for _ in range(a.reps + 1):
        pool.release(ones)
        first = torch.zeros((BATCH,), dtype=torch.int32, device=dev)
        first[0] = PROMPT
        pool.reserve(ones, 0, extra_rows=first)                               # row 0 owns 16 pages; 63 rows map its first 15
        src = pool.page_ids[0:1].expand(BATCH, -1).contiguous()
        hold.append(timed(lambda: check(lib.qs_pages_hold(*pool._state(), ptr(pool.refs), ptr(pool._scratch), ptr(take), ptr(src), 0, 0,
                                                          pool.B, pool.mb, pool.L, pool.N, pool.page_bytes, stream()), "hold")))
        unhold.append(timed(lambda: pool.release(ones)))
    say(f"    hold: 15 pages of row 0 into each of 63 rows                {med(hold[1:])} us;   the unhold of all 64 rows behind it "
        f"(16 pages freed of 961 holds) {med(unhold[1:])} us")
    for p in pools_.values():
        p.check()
    del pools_, pool

    # ---- 2. the captured step
    plain = DecodeEngine(cfg, batch=BATCH, prompt_len=PROMPT, max_new=MAX_NEW, device="cuda:0", seed=0, page_pool=N)
    counted = DecodeEngine(cfg, batch=BATCH, prompt_len=PROMPT, max_new=MAX_NEW, device="cuda:0", seed=0, page_pool=N, prefix_cache=True)
    prompt = torch.randint(0, cfg["vocab"], (BATCH * PROMPT,), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    saved = {}
    for name, eng in (("plain", plain), ("counted", counted)):
        eng.prefill_chunked(PROMPT, 256, prompt)
        eng.enable_drafting(prompt)
        saved[name] = (eng.tokens.clone(), eng.lengths.clone(), eng.history.clone(), eng.hidden.clone())
        eng.capture()

    def reset(name, eng):
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

    say(f"\n# 2. host clock around {a.replays} replays of the captured pooled step + device synchronise, us per replay; {a.reps} interleaved pairs "
        "(uncounted = what the pooled engine launched before reference counts; hit rate: none, nothing is shared in a step)")
    un, co = [], []
    for _ in range(a.reps):
        un.append(per_replay_us("plain", plain, a.replays))
        co.append(per_replay_us("counted", counted, a.replays))
    diffs = [y - x for x, y in zip(un, co)]
    say(f"    captured step   uncounted {med(un)} us   counted {med(co)} us   counted - uncounted: median of pairs "
        f"{statistics.median(diffs):+7.2f} us ({min(diffs):+.2f} .. {max(diffs):+.2f})")
    counted.check()

    # ---- 3. admit with 960 of 1 024 tokens cached
    say(f"\n# 3. admit() of 8 prompts of {PROMPT} tokens (chunk 256) into rows 0 .. 7 of the running batch: wall ms around the call + device "
        f"synchronise; {a.reps} figures each, in alternation")
    g = torch.Generator().manual_seed(3)
    common = torch.randint(0, cfg["vocab"], (960,), generator=g)
    same = [torch.cat((common, torch.randint(0, cfg["vocab"], (64,), generator=g))) for _ in range(8)]
    counted.admit([63], [torch.cat((common, torch.randint(0, cfg["vocab"], (64,), generator=g)))], chunk=256)   # row 63 computes the 15 pages
    cold, warm = [], []

    def wall(eng):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.admit(range(8), same, chunk=256)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for _ in range(a.reps + 1):
        cold.append(wall(plain))
        warm.append(wall(counted))
    hits = sum(len(counted._row_cached[r]) for r in range(8)) * 64
    say(f"    uncached (uncounted engine)   {med(cold[1:])} ms   cached (hit rate {hits} of {8 * PROMPT} prompt tokens = {hits / (8 * PROMPT):.3f})   "
        f"{med(warm[1:])} ms   = {statistics.median(warm[1:]) * 1e3 / statistics.median(co):.1f} captured steps of the live rows")
    counted.check()

    # ---- 4. serve behind a common prefix
    say(f"\n# 4. serve() over {a.requests} greedy requests behind a common prefix of {PROMPT} tokens (own tails 16 .. 256, 8 .. 128 new tokens), "
        "poll_every 8, chunk 256")
    head = torch.randint(0, cfg["vocab"], (PROMPT,), generator=g).tolist()
    tails = torch.clamp((torch.rand((a.requests,), generator=g) * 256).long(), min=16).tolist()
    news = torch.clamp((torch.rand((a.requests,), generator=g) * 128).long(), min=8).tolist()
    reqs = [(head + torch.randint(0, cfg["vocab"], (t,), generator=g).tolist(), m) for t, m in zip(tails, news)]
    asked = sum(len(p) for p, _ in reqs)
    for name, eng in (("without the cache", plain), ("with the cache   ", counted)):
        if eng.prefix is not None:                                          # start from an empty cache
            eng.release_rows(None)
            eng.evict_prefixes(N)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out, stats = eng.serve(reqs, poll_every=8, chunk=256)
        dt = time.perf_counter() - t0
        made = sum(len(r["tokens"]) for r in out)
        rate = f"hit rate {stats['hit_tokens']} of {asked} prompt tokens = {stats['hit_tokens'] / asked:.3f}" if "hit_tokens" in stats else "hit rate 0"
        say(f"    {name}: {made} tokens generated in {dt:.2f} s: {made / dt:.0f} tokens / s;   {rate};   {stats}")
        eng.check()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
