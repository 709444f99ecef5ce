"""What a fork costs and what n > 1 samples save, in ONE run (no pass / fail threshold; figures only), at the bench configuration:
Llama-3-8B shapes, KV4 (32 layers, pages of 34 816 bytes: 2.2 MB of tail pages per follower), synthetic weights, B = 64.  Method of
scripts/bench_prefix_cache.py: medians of figures taken in alternation.

  1. the fork launch pair alone (qs_pages_fork: the allocator launch and the copy grid), device events around ONE call, for 1, 7 and 63
     followers of a text of 1 000 tokens (15 whole pages shared, slot 39 of page 15 the first one still written) - beside the time the
     copied bytes take at 6.29 TB/s, read and written once each, and beside the same pages copied by torch indexed copies (one
     index_select + index_copy_ per pool tensor: 64 pairs).
  2. an admit() of one prompt of 1 024 tokens with 7 copy_rows, beside an admit of 8 copies of that prompt, on an engine with
     share_pages alone and on one with the prefix cache (emptied before every call).
  3. serve() over --requests requests of n = 4 samples, beside the same samples sent as 4 x --requests requests of n = 1: generated
     tokens / s and peak pages.

Run it under `timeout`.

    python scripts/bench_fork.py [--reps 9] [--requests 64] [--out profiles/fork.txt]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PROMPT, BATCH, MAX_NEW, TEXT = 1024, 64, 640, 1000
HBM = 6.29e12


def med(xs):
    return f"{statistics.median(xs):9.1f} ({min(xs):.1f} .. {max(xs):.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--requests", type=int, default=64)
    ap.add_argument("--skip-engine", action="store_true", help="part 1 alone")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    assert a.reps >= 3 and a.requests >= 1
    assert torch.cuda.is_available(), "bench_fork needs a GPU"
    from qserve_amd import paging
    from qserve_amd.decode import LLAMA3_8B, DecodeEngine
    dev = torch.device("cuda:0")
    cfg, lines = LLAMA3_8B, []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    L = cfg["layers"]
    mb = (PROMPT + MAX_NEW + 63) // 64 + 1
    pb = 34816                                                              # (8 KV heads x 64 slots x 64 bytes + scales and zeros)
    say(f"# {torch.cuda.get_device_name(0)}; {cfg['name']} shapes, KV4, {L} layers, page_bytes {pb}: a follower's tail pages are "
        f"{2 * L * pb / 1e6:.2f} MB; B = {BATCH}, mb = {mb}" + (f"; QS_FORK_COPY_SPLIT={os.environ['QS_FORK_COPY_SPLIT']}" if os.environ.get("QS_FORK_COPY_SPLIT") else ""))

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3

    # ---- 1. the launch pair alone
    N = 16 + BATCH
    tables = [torch.zeros((BATCH, 2, mb), dtype=torch.int64, device=dev) for _ in range(L)]
    pools = [tuple(torch.randint(0, 256, (N + 1, pb), dtype=torch.uint8, device=dev) for _ in range(2)) for _ in range(L)]
    pool = paging.PagePool(tables, pools, pb, refcounts=True)
    ones = torch.ones((BATCH,), dtype=torch.int32, device=dev)
    text = torch.zeros((BATCH,), dtype=torch.int32, device=dev)
    text[0] = TEXT
    lengths = torch.ones((BATCH,), dtype=torch.int32, device=dev)
    lengths[0] = TEXT
    say(f"\n# 1. qs_pages_fork alone (both launches), {BATCH} rows x {L} layers, a source text of {TEXT} tokens: device events around ONE "
        f"call, us; {a.reps} figures each; floor = the tail pages read once and written once at {HBM / 1e12:.2f} TB/s; torch = the same "
        f"pages by index_select + index_copy_ per pool tensor ({2 * L} pairs of launches, no allocator work)")
    for followers in (1, 7, 63):
        src = torch.full((BATCH,), -1, dtype=torch.int32, device=dev)
        src[1:1 + followers] = 0
        fork, copy = [], []
        for _ in range(a.reps + 1):
            pool.release(ones)
            pool.reserve(ones, 0, extra_rows=text)
            fork.append(timed(lambda: pool.fork(src, lengths)))
            ids = pool.page_ids[:1 + followers, (TEXT - 1) // 64].to(torch.int64)
            frm, to = ids[:1].expand(followers).contiguous(), ids[1:].contiguous()
            copy.append(timed(lambda: [t.index_copy_(0, to, t.index_select(0, frm)) for pair in pools for t in pair]))
        moved = 2 * followers * 2 * L * pb
        say(f"    {followers:2d} followers ({moved / 2e6:7.2f} MB copied)   fork {med(fork[1:])} us   floor {moved / HBM * 1e6:6.1f} us   "
            f"torch {med(copy[1:])} us")
        assert pool.owned[1:1 + followers].tolist() == [16] * followers
    pool.check(starved=True)
    del pool, pools, tables
    if a.skip_engine:
        return finish(a, lines)

    # ---- 2. admit with copy_rows
    N = BATCH * mb
    engines = dict(share=DecodeEngine(cfg, batch=BATCH, prompt_len=PROMPT, max_new=MAX_NEW, device="cuda:0", seed=0, page_pool=N, share_pages=True))
    engines["cache"] = DecodeEngine(cfg, batch=BATCH, prompt_len=PROMPT, max_new=MAX_NEW, device="cuda:0", seed=0, page_pool=N, prefix_cache=True)
    g = torch.Generator().manual_seed(3)
    prompt = torch.randint(0, cfg["vocab"], (PROMPT,), generator=g)
    for eng in engines.values():
        assert eng.page_bytes == pb and len(eng.layers) == L
        eng.enable_drafting(None)
        eng.set_stopping((), 0)
    say(f"\n# 2. admit() of one prompt of {PROMPT} tokens (chunk 256) into row 0 with copy_rows 1 .. 7, beside an admit of 8 copies of the "
        f"prompt into rows 0 .. 7: wall ms around the call + device synchronise; {a.reps} figures each, in alternation; the cache is "
        "emptied before every call")

    def wall(eng, copies):
        if eng.prefix is not None:
            eng.release_rows(None)
            eng.evict_prefixes(N)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if copies:
            eng.admit([0], [prompt], max_new_tokens=MAX_NEW, chunk=256, copy_rows=[list(range(1, 8))])
        else:
            eng.admit(range(8), [prompt] * 8, max_new_tokens=MAX_NEW, chunk=256)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for name, eng in engines.items():
        eight, forked = [], []
        for _ in range(a.reps + 1):
            eight.append(wall(eng, False))
            forked.append(wall(eng, True))
        pages = N - eng.pager.free_pages()
        say(f"    {'share_pages alone' if name == 'share' else 'with the prefix cache'}: 8 copies {med(eight[1:])} ms   1 prompt + 7 copy_rows "
            f"{med(forked[1:])} ms ({pages} pages in use behind it, {8 * ((PROMPT + 64) // 64)} behind 8 copies)")
        eng.check()
    del engines["cache"]

    # ---- 3. serve
    eng = engines["share"]
    say(f"\n# 3. serve() over {a.requests} greedy requests of n = 4 samples (prompts 256 .. 1 024 tokens, 32 .. 128 new tokens), beside the same "
        f"{4 * a.requests} samples as requests of n = 1; poll_every 8, chunk 256")
    plens = torch.clamp((torch.rand((a.requests,), generator=g) * PROMPT).long(), min=256).tolist()
    news = torch.clamp((torch.rand((a.requests,), generator=g) * 128).long(), min=32).tolist()
    prompts = [torch.randint(0, cfg["vocab"], (p,), generator=g).tolist() for p in plens]
    for name, reqs in (("n = 4", [(p, m, 4) for p, m in zip(prompts, news)]), ("n = 1", [(p, m) for p, m in zip(prompts, news) for _ in range(4)])):
        eng.release_rows(None)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out, stats = eng.serve(reqs, poll_every=8, chunk=256)
        dt = time.perf_counter() - t0
        made = sum(len(s["tokens"]) for r in out for s in r.get("samples", [r]))
        say(f"    {name}: {made} tokens generated in {dt:.2f} s: {made / dt:.0f} tokens / s;   {stats}")
        eng.check()
    finish(a, lines)


def finish(a, lines):
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
