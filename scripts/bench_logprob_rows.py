"""What log-probabilities cost (`qs_logprob_rows`, DecodeEngine.set_logprobs), in ONE run (no pass / fail threshold; figures only):

  1. the kernel on 64 rows of the Llama-3-8B vocabulary (n = 128 256) at top in {0, 5, 20}, against
       (a) `qs_sample_rows` (T = 0.8, no filter) on the same rows - a kernel of the same family that reads the row a similar number of times;
       (b) the torch path a caller would take: log_softmax(logits.float()) + topk + gather (+ the rank by a comparison and a sum);
  2. the captured step() at the bench configuration with log-probabilities off and on (top = 5).  Off issues exactly the launches a
     step issued before set_logprobs existed.

Part 1: HIP events around --iters back-to-back launches after warm-up launches of the same shape, per-launch times of --reps such
batches taken in alternation over the variants: lowest .. highest.  Part 2: host clock around --replays graph replays plus a device
synchronise, --reps figures per graph in alternation, and the median of the paired differences.  Run it under `timeout`.

    python scripts/bench_logprob_rows.py [--iters 30] [--warmup 5] [--reps 5] [--replays 50] [--out profiles/logprob_rows.txt]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N, ROWS, TOPS = 128256, 64, (0, 5, 20)
PROMPT, BATCH, MAX_NEW = 1024, 64, 640


def torch_logprobs(logits, ids, top):
    """log_softmax in float32, the chosen id's value and rank, and the top list, with tensor ops."""
    lsm = torch.log_softmax(logits.float(), dim=1)
    lp = lsm.gather(1, ids.view(-1, 1))
    rank = (lsm > lp).sum(dim=1) + 1
    if top:
        return lp, rank, torch.topk(lsm, top, dim=1)
    return lp, rank


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--skip-step", action="store_true", help="part 1 only (no 8B engine)")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    assert a.iters >= 10 and a.reps >= 3 and a.replays >= 10
    assert torch.cuda.is_available(), "bench_logprob_rows needs a GPU"
    from qserve_amd.logprobs import logprob_rows, new_logs
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

    say(f"# {torch.cuda.get_device_name(0)}; 1. fp16 logits [{ROWS}, {N}] (standard normal x 3); HIP events around {a.iters} back-to-back launches, "
        f"us per launch; {a.reps} such figures per variant in alternation: lowest .. highest")
    logits = (torch.randn((ROWS, N), device=dev, generator=torch.Generator(device=dev).manual_seed(ROWS)) * 3.0).half()
    ids = torch.randint(0, N, (ROWS,), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    drawn = torch.empty((ROWS,), dtype=torch.int64, device=dev)
    keys = torch.arange(ROWS, dtype=torch.int64, device=dev)
    summary = []
    for top in TOPS:
        out = tuple(t.squeeze(1) for t in new_logs(ROWS, 1, top, dev))
        variants = {
            "qs_logprob_rows": lambda: logprob_rows(logits, ids, 1.0, top, out=out),
            "qs_sample_rows (T=0.8)": lambda: sample_rows(logits, drawn, 0.8, 0, 1.0, seed=1, row_keys=keys),
            "torch log_softmax + topk + gather": lambda: torch_logprobs(logits, ids, top),
        }
        t = {v: [] for v in variants}
        for _ in range(a.reps):
            for v, fn in variants.items():
                t[v].append(per_launch_us(fn))
        say(f"\n  top={top}:")
        for v, x in t.items():
            say(f"    {v:36s} {min(x):10.1f} .. {max(x):10.1f} us")
        med = {v: statistics.median(x) for v, x in t.items()}
        summary.append(f"    top={top:<3d}: logprob_rows {med['qs_logprob_rows']:9.1f} us = x{med['qs_logprob_rows'] / med['qs_sample_rows (T=0.8)']:6.2f} of "
                       f"sample_rows ({med['qs_sample_rows (T=0.8)']:8.1f} us), x{med['qs_logprob_rows'] / med['torch log_softmax + topk + gather']:6.3f} of the "
                       f"torch path ({med['torch log_softmax + topk + gather']:9.1f} us)")
    say("\n# summary of 1.: medians, and qs_logprob_rows as a multiple of each yardstick (below 1 = faster)")
    for s in summary:
        say(s)
    del logits
    torch.cuda.empty_cache()

    if not a.skip_step:
        from qserve_amd.decode import LLAMA3_8B, DecodeEngine
        say(f"\n# 2. {LLAMA3_8B['name']} shapes, KV4, B = {BATCH}, prompt {PROMPT}: the captured step(), log-probabilities off / on (top = 5); host clock "
            f"around {a.replays} replays + device synchronise, us per replay; {a.reps} figures per graph in alternation")
        prompt = torch.randint(0, LLAMA3_8B["vocab"], (BATCH * PROMPT,), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        eng = DecodeEngine(LLAMA3_8B, batch=BATCH, prompt_len=PROMPT, max_new=MAX_NEW, device="cuda:0", seed=0)
        eng.prefill_chunked(PROMPT, 256, prompt)
        state0 = (eng.tokens.clone(), eng.lengths.clone(), eng.hidden.clone())

        def reset():
            eng.tokens.copy_(state0[0])
            eng.lengths.copy_(state0[1])
            eng.hidden.copy_(state0[2])
            eng._len_bound = PROMPT + 1

        graphs = {}
        eng.capture()
        graphs["off"] = eng.graph
        reset()
        eng.set_logprobs(top=5)
        eng.capture()
        graphs["on"] = eng.graph

        def per_replay_us(g):
            reset()
            for _ in range(3):
                g.replay()
            reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.replays):
                g.replay()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e6 / a.replays

        off, on = [], []
        for _ in range(a.reps):
            off.append(per_replay_us(graphs["off"]))
            on.append(per_replay_us(graphs["on"]))
        diffs = [y - x for x, y in zip(off, on)]
        say(f"    captured step  logprobs off {statistics.median(off):9.1f} us ({min(off):.1f} .. {max(off):.1f})   on {statistics.median(on):9.1f} us "
            f"({min(on):.1f} .. {max(on):.1f})   on - off: median of pairs {statistics.median(diffs):+7.2f} us ({min(diffs):+.2f} .. {max(diffs):+.2f})")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
