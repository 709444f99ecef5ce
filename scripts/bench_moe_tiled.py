"""The two forms of the grouped W4A8 GEMM (qserve_amd.moe.grouped_gemm: the weight-streaming kernel and the compute-bound tile of
csrc/gemm_w4a8_moe_tiled.hip) at Mixtral-8x7B expert shapes - gate_up 4096 -> 28672 (rows gathered through row_src), down 14336 -> 4096,
E = 8, k = 2 - in ONE run (figures only, no pass / fail threshold):

  1. sweep: expected rows per expert ceil(P / E) over 32 .. 2048 under a seeded routing, streaming against tiled on the same tensors, in
     alternation; the spread of the sweep is the largest (highest - lowest) / median of any figure.  The planner's threshold
     (csrc/moe_plan.h TILED_MIN_ROWS) is read from this table: the smallest row count from which the tile wins at BOTH shapes by more
     than that spread;
  2. P = 2 048, 16 384 and 131 072 sorted rows: both forms and E dense launches on pre-gathered rows (the ceiling the dense tiles set;
     not an option for the engine - it would have to read the routing back), with the achieved POPS (2 P N K operations);
  3. prefill_chunked of 8 x 1 024 tokens (chunk 1 024: P = 16 384 per layer) on MIXTRAL_8X7B cut to --layers layers, the entries forced
     to stream (what the parent commit ran) against the tile wherever it serves (the planner's choice at this P once the threshold of
     part 1 is in csrc/moe_plan.h; the decode step is not part of this figure).

Parts 1 and 2: `iters` calls captured in one hipGraph after warm-up calls, HIP events around three replays, --reps figures per variant in
alternation: median (lowest .. highest).  Part 3: a host clock around a call that ends in a device synchronise.  Outputs of the forms are
compared bit for bit at every size timed.  Run it under `timeout`.

    python scripts/bench_moe_tiled.py [--reps 5] [--layers 8] [--group-size -1] [--parts 123] [--out profiles/moe_tiled.txt]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

E, TOPK, HID, INTER = 8, 2, 4096, 14336


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--group-size", type=int, default=-1, choices=(-1, 128))
    ap.add_argument("--parts", default="123")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    assert a.reps >= 3 and torch.cuda.is_available(), "bench_moe_tiled needs a GPU and at least 3 repeats"
    import qserve_backend.qgemm_w4a8_per_chn as gemm_chn
    import qserve_backend.qgemm_w4a8_per_group as gemm_grp
    from qserve_amd import decode as D
    from qserve_amd import moe
    from qserve_amd._lib import lib
    dev = torch.device("cuda:0")
    per_chn = a.group_size == -1
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
        if a.out:                                         # (kept current: a run cut short leaves what it measured)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    def graph_of(fn, iters):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(iters):
                fn()
        return g

    def timed_us(g, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        g.replay()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(3):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / (3 * iters)

    def alternated(fns, iters):
        graphs = {n: graph_of(f, iters) for n, f in fns.items()}
        got = {n: [] for n in graphs}
        for _ in range(a.reps):
            for n, g in graphs.items():
                got[n].append(timed_us(g, iters))
        return {n: (statistics.median(v), min(v), max(v)) for n, v in got.items()}

    fmt = lambda r: f"{r[0]:9.1f} us ({r[1]:.1f} .. {r[2]:.1f})"   # noqa: E731
    gen = torch.Generator(device=dev).manual_seed(0)
    shapes = (("gate_up", 2 * INTER, HID, True), ("down", HID, INTER, False))
    lins = {name: moe.MoELinear(E, N, K, a.group_size, dev, gen) for name, N, K, _ in shapes}
    spreads = []

    def problem(name, N, K, gathered, T):
        """Both forms (and the dense loop) on one seeded routing of T tokens: {variant: callable}, after a bit-for-bit comparison."""
        P, lin = T * TOPK, lins[name]
        logits = torch.randn((T, E), device=dev, generator=gen).half()
        _, _, offs, ptok, _ = moe.route(logits, TOPK)
        rows = T if gathered else P
        x = torch.randint(-127, 128, (rows, K), dtype=torch.int8, device=dev, generator=gen)
        xs = (torch.rand((rows,), device=dev, generator=gen) * 0.01 + 0.001).half()
        xsum = torch.randn((rows,), device=dev, generator=gen).half() if per_chn else None
        src = ptok if gathered else None
        outs = {f: torch.empty((P, N), dtype=torch.float16, device=dev) for f in ("streaming", "tiled", "dense")}
        gx, gs = (x[ptok.long()].contiguous(), xs[ptok.long()].contiguous()) if gathered else (x, xs)
        gsum = (xsum[ptok.long()].contiguous() if gathered else xsum) if per_chn else None
        bounds = offs.tolist()
        experts = [(lin.expert(e), bounds[e], bounds[e + 1]) for e in range(E) if bounds[e + 1] > bounds[e]]

        def dense():
            for w, lo, hi in experts:
                if per_chn:
                    gemm_chn.gemm_forward_cuda(gx[lo:hi], w["qweight"], w["s1_scales"], gs[lo:hi], w["s1_szeros"], gsum[lo:hi], outs["dense"][lo:hi])
                else:
                    gemm_grp.gemm_forward_cuda(gx[lo:hi], w["qweight"], w["s2_zeros"], w["s2_scales"], w["s1_scales"], gs[lo:hi], outs["dense"][lo:hi])

        fns = {f: (lambda f=f: moe.grouped_gemm(x, xs, xsum, offs, lin, outs[f], row_src=src, form=f)) for f in ("streaming", "tiled")}
        fns["dense"] = dense
        for f in fns.values():
            f()
        torch.cuda.synchronize()
        for f in ("tiled", "dense"):
            assert torch.equal(outs[f].view(torch.int16), outs["streaming"].view(torch.int16)), f"{name} P={P}: {f} differs from streaming"
        return fns, torch.diff(offs).tolist()

    say(f"bench_moe_tiled: Mixtral-8x7B expert shapes, E = {E}, k = {TOPK}, {'per-channel' if per_chn else 'per-group-128'} weights; "
        f"{a.reps} alternated repeats: median (lowest .. highest); planner threshold now: tiled from "
        f"{next((r for r in range(1, 4097) if moe.gemm_form(r * E, E, 2 * INTER, HID) == 'tiled'), None)} rows per expert")
    if "1" in a.parts:
        say("1. sweep over the expected rows per expert (seeded routing), streaming against tiled")
        for name, N, K, gathered in shapes:
            for r in (32, 64, 128, 256, 512, 1024, 2048):
                fns, counts = problem(name, N, K, gathered, r * E // TOPK)
                del fns["dense"]
                res = alternated(fns, max(3, min(20, 2048 // r)))
                spreads += [(v[2] - v[1]) / v[0] for v in res.values()]
                say(f"    {name:8s} rows/expert {r:5d} (P = {r * E:6d}): streaming {fmt(res['streaming'])}  tiled {fmt(res['tiled'])}  "
                    f"tiled / streaming = {res['tiled'][0] / res['streaming'][0]:.3f}")
        say(f"    run-to-run spread of the sweep: largest (highest - lowest) / median = {max(spreads):.3f}")
    if "2" in a.parts:
        say("2. both forms and E dense launches on pre-gathered rows; POPS = 2 P N K / time")
        for name, N, K, gathered in shapes:
            for P in (2048, 16384, 131072):
                fns, counts = problem(name, N, K, gathered, P // TOPK)
                res = alternated(fns, 3 if P > 16384 else 6)
                pops = lambda r: 2.0 * P * N * K / (r[0] * 1e-6) / 1e15   # noqa: E731
                say(f"    {name:8s} P = {P:6d} (rows per expert {min(counts)} .. {max(counts)})")
                for f in ("streaming", "tiled", "dense"):
                    say(f"        {f:10s} {fmt(res[f])}  {pops(res[f]):.2f} POPS")
    if "3" in a.parts:
        cfg = dict(D.MIXTRAL_8X7B, layers=a.layers)
        eng = D.DecodeEngine(cfg, batch=8, prompt_len=1024, max_new=8, device="cuda:0", group_size=a.group_size)
        say(f"3. prefill_chunked, 8 x 1 024 tokens, chunk 1 024, MIXTRAL_8X7B cut to {a.layers} of 32 layers + lm_head; grouped GEMM form for "
            f"P = 16 384: {moe.gemm_form(16384, E, 2 * INTER, HID)} (gate_up), {moe.gemm_form(16384, E, HID, INTER)} (down)")
        got = {"streaming (the parent commit's kernel)": [], "the tile wherever it serves": []}
        eng.prefill_chunked(1024, 1024)
        for _ in range(a.reps):
            for n, hook in zip(got, (0, 1)):
                lib.qs_set_moe_gemm_form(hook)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                eng.prefill_chunked(1024, 1024)
                torch.cuda.synchronize()
                got[n].append((time.perf_counter() - t0) * 1e3)
        lib.qs_set_moe_gemm_form(-1)
        for n, v in got.items():
            say(f"    {n:40s} {statistics.median(v):8.2f} ms ({min(v):.2f} .. {max(v):.2f})")


if __name__ == "__main__":
    main()
