"""What scoring prompt rows costs (`qs_score_rows`, logprobs.score_rows), in ONE run (no pass / fail threshold; figures only): the kernel
against the torch path a caller would otherwise take, on the same commit, at Llama-3-8B head shapes (K = 4 096, V = 128 256) with 512 /
2 048 / 8 192 rows and at one K = 8 192 shape:

    torch path   per chunk of --chunk-rows rows: torch.matmul(hidden, lm_head.t()) -> fp16 logits, log_softmax in float32, gather of the
                 target, argmax (the chunk keeps the logit matrices of large row counts inside a bounded footprint)
    score_rows   one call over all rows: no logit matrix; a 16-byte record per row and vocabulary split

Per variant: time (HIP events around back-to-back calls after warm-up calls of the same shape; the number of calls is chosen so that a
window lasts about --window seconds; --reps windows per variant in alternation: median, lowest .. highest), the fp16 rate 2 rows V K / time
against the dense fp16 matrix peak (2 500 TFLOP/s), and the peak device memory allocated beyond the inputs during a call (torch's
allocator statistics; for score_rows that is its outputs plus its workspace).  Before timing, the two paths are compared on the shape.

    python scripts/bench_score_rows.py [--reps 5] [--window 0.3] [--chunk-rows 2048] [--out profiles/score_rows.txt]
"""
import argparse
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

V = 128256
SHAPES = [(512, 4096), (2048, 4096), (8192, 4096), (2048, 8192)]          # (rows, K)
FP16_PEAK_TFLOPS = 2500.0


def torch_score(hidden, lm_head, targets, chunk):
    """matmul in row chunks, float32 log_softmax, gather, argmax -> (lp [rows], greedy [rows])."""
    lps, greedy = [], []
    for r0 in range(0, hidden.size(0), chunk):
        logits = torch.matmul(hidden[r0:r0 + chunk], lm_head.t())
        lsm = torch.log_softmax(logits.float(), dim=1)
        lps.append(lsm.gather(1, targets[r0:r0 + chunk].long().view(-1, 1)).squeeze(1))
        greedy.append(logits.argmax(dim=1))
    return torch.cat(lps), torch.cat(greedy)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3, help="seconds of back-to-back calls per timed window")
    ap.add_argument("--chunk-rows", type=int, default=2048)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    assert a.reps >= 3 and a.window > 0 and a.chunk_rows >= 1
    assert torch.cuda.is_available(), "bench_score_rows needs a GPU"
    from qserve_amd.logprobs import score_plan, score_rows
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def window_ms(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / calls

    def extra_mib(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        del out
        return peak / 2 ** 20

    say(f"# {torch.cuda.get_device_name(0)}; V = {V}; hidden standard normal, lm_head x 0.02, fp16; torch path in chunks of {a.chunk_rows} rows; "
        f"ms per call, {a.reps} windows of ~{a.window} s per variant in alternation: median (lowest .. highest); rate = 2 rows V K / median; "
        f"peak = {FP16_PEAK_TFLOPS:.0f} TFLOP/s")
    table = []
    for rows, K in SHAPES:
        g = torch.Generator(device=dev).manual_seed(rows + K)
        hidden = torch.randn((rows, K), device=dev, generator=g).half()
        lm_head = (torch.randn((V, K), device=dev, generator=g) * 0.02).half()
        targets = torch.randint(0, V, (rows,), device=dev, generator=g).to(torch.int32)
        variants = {"score_rows": lambda: score_rows(hidden, lm_head, targets), "torch": lambda: torch_score(hidden, lm_head, targets, a.chunk_rows)}
        plan = score_plan(rows, V, K)
        # the two paths on this shape (torch rounds its logits to fp16, so the difference is dominated by that rounding)
        (lp_k, gr_k), (lp_t, gr_t) = variants["score_rows"](), variants["torch"]()
        say(f"\n  rows={rows} K={K}: plan {plan['row_tiles']} row tiles x {plan['splits']} splits of {plan['tiles_per_split']} tiles, workspace "
            f"{plan['workspace_bytes'] / 2 ** 20:.2f} MiB; max |lp - torch lp| = {(lp_k - lp_t).abs().max().item():.2e}, greedy equal on "
            f"{int((gr_k.long() == gr_t).sum())} of {rows} rows")
        del lp_k, gr_k, lp_t, gr_t
        mem = {v: extra_mib(fn) for v, fn in variants.items()}
        mem["score_rows"] += plan["workspace_bytes"] / 2 ** 20            # (kept between calls: it exists since the comparison above)
        calls = {}
        for v, fn in variants.items():                                    # warm-up, and the number of calls of a window
            fn()
            calls[v] = max(3, min(200, math.ceil(a.window * 1e3 / window_ms(fn, 2))))
        t = {v: [] for v in variants}
        for _ in range(a.reps):
            for v, fn in variants.items():
                t[v].append(window_ms(fn, calls[v]))
        flop = 2.0 * rows * V * K
        for v, x in t.items():
            med = statistics.median(x)
            say(f"    {v:12s} {med:9.3f} ms ({min(x):9.3f} .. {max(x):9.3f}; {calls[v]:3d} calls per window)  {flop / med / 1e9:7.1f} TFLOP/s = "
                f"{flop / med / 1e9 / FP16_PEAK_TFLOPS:.3f} of peak   extra memory {mem[v]:9.1f} MiB")
        table.append((rows, K, statistics.median(t["score_rows"]), statistics.median(t["torch"]), mem["score_rows"], mem["torch"]))
        del hidden, lm_head, targets, variants
        torch.cuda.empty_cache()
    say("\n# summary: medians; time of score_rows as a multiple of the torch path (below 1 = faster), extra memory of each")
    for rows, K, tk, tt, mk, mt in table:
        say(f"    rows={rows:5d} K={K}: score_rows {tk:9.3f} ms, torch {tt:9.3f} ms, x{tk / tt:6.3f};  memory {mk:8.1f} MiB against {mt:9.1f} MiB")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
