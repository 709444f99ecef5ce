"""What the mixture-of-experts path costs (qserve_amd.moe, DecodeEngine on MIXTRAL_8X7B), in ONE run (no pass / fail threshold; figures
only):

  1. Mixtral-8x7B expert shapes - gate_up 4096 -> 28672, down 14336 -> 4096, E = 8, k = 2 - at T = 64 tokens (P = 128 sorted rows) under a
     seeded routing: the grouped GEMM against (a) the bytes' floor: the ACTIVE experts' weight bytes (an expert with no row is not read)
     over the 6.29 TB/s a float4 copy reaches on this chip (8.0 TB/s is the data sheet's figure) and (b) E dense launches of the same
     library on the gathered rows, one per non-empty expert - what a host loop costs even if it knew the routing (it does not: the
     counts would have to be read back);
  2. route and combine at the same sizes;
  3. the captured step of MIXTRAL_8X7B at B = 64 (KV4, prompt 1 024), --layers layers (all 32 need ~25 GB of synthetic weights), and
     its time per layer.

Parts 1 and 2: --iters calls captured in one hipGraph after warm-up calls (device time: no host work between the launches), HIP events
around three replays, --reps such figures per variant in alternation: median (lowest .. highest).  Part 3: a host clock around
--replays replays that end in a device synchronise, --reps times.  Run it under `timeout`.

    python scripts/bench_moe.py [--iters 20] [--reps 5] [--replays 30] [--layers 8] [--skip-step] [--out profiles/moe.txt]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

T, E, TOPK, HID, INTER = 64, 8, 2, 4096, 14336
COPY_RATE = 6.29e12   # bytes / s: the measured float4 copy rate of the chip (8.0e12 is the data sheet's)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--replays", type=int, default=30)
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    assert a.iters >= 5 and a.reps >= 3 and a.replays >= 5
    assert torch.cuda.is_available(), "bench_moe needs a GPU"
    import qserve_backend.qgemm_w4a8_per_chn as gemm_chn
    from qserve_amd import decode as D
    from qserve_amd import moe
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def graph_of(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(a.iters):
                fn()
        return g

    def timed_us(g):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        g.replay()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(3):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / (3 * a.iters)

    def alternated(graphs):
        """{name: graph} -> {name: (median, lowest, highest)} us per call, the variants measured in alternation."""
        got = {n: [] for n in graphs}
        for _ in range(a.reps):
            for n, g in graphs.items():
                got[n].append(timed_us(g))
        return {n: (statistics.median(v), min(v), max(v)) for n, v in got.items()}

    fmt = lambda r: f"{r[0]:8.1f} us ({r[1]:.1f} .. {r[2]:.1f})"   # noqa: E731
    gen = torch.Generator(device=dev).manual_seed(0)
    say(f"bench_moe: Mixtral-8x7B expert shapes, T = {T} tokens, E = {E}, k = {TOPK}, P = {T * TOPK} sorted rows; {a.iters} calls per graph, "
        f"{a.reps} alternated repeats: median (lowest .. highest)")
    logits = torch.randn((T, E), device=dev, generator=gen).half()
    ids, w, offs, ptok, ppos = moe.route(logits, TOPK)
    counts = torch.diff(offs).tolist()
    active = sum(1 for c in counts if c)
    say(f"seeded routing: rows per expert {counts} ({active} active experts)")
    P = T * TOPK
    for name, N, K, gathered in (("gate_up", 2 * INTER, HID, True), ("down", HID, INTER, False)):
        lin = moe.MoELinear(E, N, K, -1, dev, gen)
        rows = T if gathered else P
        x = torch.randint(-127, 128, (rows, K), dtype=torch.int8, device=dev, generator=gen)
        xs = (torch.rand((rows,), device=dev, generator=gen) * 0.01 + 0.001).half()
        xsum = torch.zeros((rows,), dtype=torch.float16, device=dev)
        out = torch.empty((P, N), dtype=torch.float16, device=dev)
        src = ptok if gathered else None
        gx = (x[ptok.long()] if gathered else x).contiguous()
        gs = (xs[ptok.long()] if gathered else xs).contiguous()
        gsum = torch.zeros((P,), dtype=torch.float16, device=dev)
        dense_out = torch.empty((P, N), dtype=torch.float16, device=dev)
        bounds = offs.tolist()
        experts = [(lin.expert(e), bounds[e], bounds[e + 1]) for e in range(E) if bounds[e + 1] > bounds[e]]

        def grouped():
            moe.grouped_gemm(x, xs, xsum, offs, lin, out, row_src=src)

        def dense_loop():
            for wts, lo, hi in experts:
                gemm_chn.gemm_forward_cuda(gx[lo:hi], wts["qweight"], wts["s1_scales"], gs[lo:hi], wts["s1_szeros"], gsum[lo:hi], dense_out[lo:hi])

        grouped()
        dense_loop()
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int16), dense_out.view(torch.int16)), "grouped and dense outputs differ"
        res = alternated({"grouped": graph_of(grouped), "dense": graph_of(dense_loop)})
        floor_us = active * N * (K // 2) / COPY_RATE * 1e6
        plan = moe.gemm_plan(P, E, N, K)
        say(f"{name:8s} N = {N}, K = {K}, plan (mt, waves, row blocks, units) = {plan}")
        say(f"    grouped GEMM (one launch)            {fmt(res['grouped'])}")
        say(f"    {active} dense launches, gathered rows     {fmt(res['dense'])}")
        say(f"    bytes' floor ({active} experts' weights at 6.29 TB/s) {floor_us:8.1f} us -> grouped = {res['grouped'][0] / floor_us:.2f} x the floor")
        del lin, out, dense_out
    y = torch.randn((P, HID), device=dev, generator=gen).half()
    comb = torch.empty((T, HID), dtype=torch.float16, device=dev)
    bufs = moe.route_buffers(T, E, TOPK, dev)
    res = alternated({"route": graph_of(lambda: moe.route(logits, TOPK, out=bufs)), "combine": graph_of(lambda: moe.combine(comb, y, w, ppos))})
    say(f"route   [T = {T}, E = {E}, k = {TOPK}] (one launch)   {fmt(res['route'])}")
    say(f"combine [T = {T}, N = {HID}, k = {TOPK}]              {fmt(res['combine'])}")
    if a.skip_step:
        say("captured MIXTRAL_8X7B step: not measured (--skip-step)")
    else:
        cfg = dict(D.MIXTRAL_8X7B, layers=a.layers)
        eng = D.DecodeEngine(cfg, batch=64, prompt_len=1024, max_new=a.replays * (a.reps + 2) + 8, device="cuda:0")
        eng.prefill_cache(1024)
        eng.capture()
        times = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.replays):
                eng.run()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) / a.replays * 1e6)
        med = statistics.median(times)
        say(f"captured MIXTRAL_8X7B step, B = 64, prompt 1 024, {a.layers} of 32 layers + lm_head: {med:8.1f} us ({min(times):.1f} .. "
            f"{max(times):.1f}) per step, {a.replays} replays per figure")
        say(f"    ({med / a.layers:.1f} us per layer if the head is counted in; a step over all 32 layers: not measured)")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
