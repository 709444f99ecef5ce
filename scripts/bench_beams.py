"""What beam search costs, in ONE run (no pass / fail threshold; figures only), at the bench configuration: Llama-3-8B shapes, KV4,
synthetic weights, B = 64 = 16 groups x 4.  Device events around one call, warmed up, the sides of a comparison taken in alternation;
every line gives the median and the range of its figures.

  1. qs_beam_select (both launches) at 64 x 128 256, W = 4, beside qs_logprob_rows(top = 4) and qs_argmax_rows on the same rows.
  2. qs_rows_move over the engine's per-row text state (lengths, history, prompt_lens, limit_lens, finished) with every second row moved.
  3. the unhold + fork pair on a round where nothing moves (a mask of zeros, sources of -1).
  4. the captured beam step beside the same build's captured greedy pooled step, and - with --parent-decode FILE, the parent commit's
     qserve_amd/decode.py, loaded over the same library - beside the parent's captured greedy pooled step.

Run it under `timeout`.

    python scripts/bench_beams.py [--reps 15] [--parent-decode FILE] [--out profiles/beams.txt]
"""
import argparse
import importlib.util
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BATCH, W, VOCAB, PROMPT, MAX_NEW = 64, 4, 128256, 512, 256
PARENT = "greedy step (parent's decode.py)"


def med(xs):
    return f"{statistics.median(xs):9.1f} ({min(xs):.1f} .. {max(xs):.1f})"


def timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def alternate(sides, reps):
    """sides: name -> call; -> name -> the figures of `reps` rounds behind one warm-up round, the sides in turn within a round."""
    out = {k: [] for k in sides}
    for _ in range(reps + 1):
        for k, fn in sides.items():
            out[k].append(timed(fn))
    return {k: v[1:] for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--skip-engine", action="store_true", help="parts 1 .. 3 alone")
    ap.add_argument("--parent-decode", default=None, help="the parent commit's qserve_amd/decode.py, for the beams-off comparison")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    assert a.reps >= 3
    assert torch.cuda.is_available(), "bench_beams needs a GPU"
    from qserve_amd import beams, logprobs, paging
    from qserve_amd import decode as D
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"# {torch.cuda.get_device_name(0)}; device events around one call, us; {a.reps} figures per line behind one warm-up, the sides of a "
        "comparison in alternation: median (min .. max)")

    # ---- 1. the selection beside the passes it restates
    g = torch.Generator(device=dev).manual_seed(1)
    logits = (torch.randn((BATCH, VOCAB), device=dev, generator=g) * 3).to(torch.float16)
    cum = -torch.rand((BATCH,), device=dev, generator=g)
    fin = torch.zeros((BATCH,), dtype=torch.int32, device=dev)
    toks = torch.zeros((BATCH,), dtype=torch.int64, device=dev)
    out = beams.select(logits, cum, fin, toks, W)
    logs = logprobs.new_logs(BATCH, 1, W, dev)
    lp_out = tuple(t.squeeze(1) for t in logs)
    am = torch.empty((BATCH,), dtype=torch.int64, device=dev)
    res = alternate({"beam_select": lambda: beams.select(logits, cum, fin, toks, W, out=out),
                     "logprob_rows(top=4)": lambda: logprobs.logprob_rows(logits, toks, 1.0, W, out=lp_out),
                     "argmax_rows": lambda: D.argmax_rows_(logits, am)}, a.reps)
    say(f"\n# 1. {BATCH} x {VOCAB} fp16 logits ({BATCH * VOCAB * 2 / 1e6:.1f} MB), W = {W}: qs_beam_select runs the passes of the "
        "log-probability launch (maximum, weights + coarse histogram, fine histogram, selection) and one merge wave per group")
    for k, v in res.items():
        say(f"    {k:22s} {med(v)} us")
    say(f"    beam_select - logprob_rows(top=4), medians: {statistics.median(res['beam_select']) - statistics.median(res['logprob_rows(top=4)']):.1f} us "
        "(the merge launch and the second launch's start; the first launch skips the rank's two counts)")

    # ---- 2. the row move
    cap = PROMPT + MAX_NEW
    rows = [torch.zeros((BATCH,), dtype=torch.int32, device=dev), torch.zeros((BATCH, cap), dtype=torch.int32, device=dev),
            torch.zeros((BATCH,), dtype=torch.int32, device=dev), torch.zeros((BATCH,), dtype=torch.int32, device=dev),
            torch.zeros((BATCH,), dtype=torch.int32, device=dev)]
    err = torch.zeros((1,), dtype=torch.int32, device=dev)
    half = torch.arange(BATCH, dtype=torch.int32, device=dev) // 2 * 2       # every odd row becomes the even row in front of it
    none = torch.arange(BATCH, dtype=torch.int32, device=dev)
    res = alternate({"every second row moves": lambda: beams.move_rows(half, rows, err), "nothing moves": lambda: beams.move_rows(none, rows, err)},
                    a.reps)
    say(f"\n# 2. qs_rows_move over lengths, history [{BATCH}, {cap}] int32, prompt_lens, limit_lens, finished: one launch of {len(rows)} x {BATCH} workgroups")
    for k, v in res.items():
        say(f"    {k:22s} {med(v)} us")
    assert int(err) == 0

    # ---- 3. unhold + fork where nothing moves
    cfg = D.LLAMA3_8B
    L, pb = cfg["layers"], 34816
    mb = (cap + 63) // 64 + 1
    N = BATCH * mb
    tables = [torch.zeros((BATCH, 2, mb), dtype=torch.int64, device=dev) for _ in range(L)]
    pools = [tuple(torch.zeros((N + 1, pb), dtype=torch.uint8, device=dev) for _ in range(2)) for _ in range(L)]
    pool = paging.PagePool(tables, pools, pb, refcounts=True)
    text = torch.full((BATCH,), PROMPT, dtype=torch.int32, device=dev)
    pool.reserve(torch.ones_like(text), 0, extra_rows=text)
    zeros, minus = torch.zeros_like(text), torch.full_like(text, -1)
    res = alternate({"unhold + fork": lambda: (pool.release(zeros), pool.fork(minus, text, finished=fin))}, a.reps)
    say(f"\n# 3. the regroup's pool launches on a round where nothing moves ({BATCH} rows x {L} layers, mb = {mb}): qs_pages_unhold and both "
        "launches of qs_pages_fork")
    say(f"    {'unhold + fork':22s} {med(res['unhold + fork'])} us")
    pool.check(starved=True)
    del pool, pools, tables
    if a.skip_engine:
        return finish(a, lines)

    # ---- 4. the captured steps
    def engine(mod, width):
        e = mod.DecodeEngine(cfg, batch=BATCH, prompt_len=PROMPT, max_new=MAX_NEW, device="cuda:0", seed=0, page_pool=N, share_pages=True)
        e.enable_drafting(None)
        e.set_stopping((), 0)
        if width:
            e.set_beams(width)
        gen = torch.Generator().manual_seed(3)
        for grp in range(BATCH // W):
            e.admit([grp * W], [torch.randint(0, cfg["vocab"], (PROMPT,), generator=gen)], max_new_tokens=MAX_NEW, chunk=256,
                    copy_rows=[list(range(grp * W + 1, grp * W + W))])
        e.capture(piecewise=False)
        return e

    sides = {"beam step": engine(D, W), "greedy step (this build)": engine(D, None)}
    if a.parent_decode:
        spec = importlib.util.spec_from_file_location("qserve_amd._decode_parent", a.parent_decode)
        parent = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(parent)
        sides[PARENT] = engine(parent, None)
    # two alternations of two sides each: a step is timed behind its own counterpart, not behind a third engine's round (whose
    # tail copies leave the caches in another state); the second one swaps its order half-way
    res = alternate({k: sides[k].run for k in ("beam step", "greedy step (this build)")}, a.reps)
    say(f"\n# 4. one captured pooled step, {cfg['name']} shapes, B = {BATCH} = {BATCH // W} groups x {W}, texts of {PROMPT} + tokens: graph replay")
    for k, v in res.items():
        say(f"    {k:34s} {med(v)} us")
    base = statistics.median(res["greedy step (this build)"])
    say(f"    beam step - greedy step, medians: {statistics.median(res['beam step']) - base:.1f} us")
    if a.parent_decode:
        ours, theirs = "greedy step (this build)", PARENT
        first = alternate({k: sides[k].run for k in (ours, theirs)}, a.reps)
        second = alternate({k: sides[k].run for k in (theirs, ours)}, a.reps)
        both = {k: first[k] + second[k] for k in (ours, theirs)}
        say("  beams off against the parent commit's decode.py over the same library (the launches are the same), in alternation, each side "
            "first in half of the rounds:")
        for k, v in both.items():
            say(f"    {k:34s} {med(v)} us")
        say(f"    this build - parent, medians: {statistics.median(both[ours]) - statistics.median(both[theirs]):.1f} us")
    else:
        say("    greedy step against the parent commit: not measured (no --parent-decode)")
    moved = sides["beam step"]._beam.moved
    say(f"    rows moved in the last beam round: {int(moved.sum())} of {BATCH}")
    for e in sides.values():
        e.check()
    finish(a, lines)


def finish(a, lines):
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
