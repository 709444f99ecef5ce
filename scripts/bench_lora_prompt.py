"""The prompt form of the LoRA row update (`lora.lora_rows(form="prompt")`, csrc/lora_prompt.hip) against the rows form, in ONE run (no
pass / fail threshold; figures only - csrc/lora_plan.h takes PROMPT_MIN_ROWS_PER_SEQ and PROMPT_MIN_ROWS from section 1):

  1. per call, rows form and prompt form in alternation, on the four linears of a Llama-3-8B layer (qkv 4096 -> 6144 in three segments,
     o 4096 -> 4096, gate_up 4096 -> 28672 in two, down 14336 -> 4096), r = 16, 8 adapters, rows_per_seq 16 .. 1 024 at T = 4 096 and
     16 384; beside each the time the call's bytes would take at the copy rate measured in the same run (distinct adapters' A and B, x,
     x_scale, out read and written, the float32 partial planes written and read);
  2. one line each for r = 64 and for 64 distinct adapters (T = 16 384, rows_per_seq = 256, qkv and gate_up);
  3. prefill_chunked of 64 x 1 024 tokens in chunks of 256 on Llama-3-8B shapes with LoRA off, with every id -1 and under eight
     r = 16 adapters, and
  4. a 64-node verify_tree at B = 64 under eight adapters -
     both with the planner's form and with `lora.rows_form` answering "rows", in alternation, eager, host clock + synchronise.

Parts 1 and 2: --iters calls captured in one hipGraph after warm-up calls of the same shape, HIP events around three replays; --reps
such figures per form in alternation: median (lowest .. highest).  Run it under `timeout`.

    python scripts/bench_lora_prompt.py [--iters 20] [--reps 3] [--skip-engine] [--out profiles/lora_prompt.txt]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = dict(qkv=(4096, 6144, (4096, 5120, 6144)), o=(4096, 4096, (4096,)), gate_up=(4096, 28672, (14336, 28672)), down=(14336, 4096, (4096,)))
SWEEP = (16, 32, 64, 128, 256, 1024)
PROMPT, BATCH, MAX_NEW, CHUNK, NODES = 1024, 64, 640, 256, 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-engine", action="store_true", help="parts 1 and 2 only (no 8B engine)")
    ap.add_argument("--out", default=None, help="also write the report to this file (line by line, as it is measured)")
    a = ap.parse_args()
    assert a.reps >= 3 and torch.cuda.is_available(), "bench_lora_prompt needs a GPU and at least three figures per variant"
    from qserve_amd import lora as loramod
    dev = torch.device("cuda:0")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").close()

    def say(s=""):
        print(s, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(s + "\n")

    def timed_us(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n

    def fig(v, unit="us"):
        return f"{statistics.median(v):9.1f} {unit} ({min(v):.1f} .. {max(v):.1f})"

    src = torch.empty((1 << 28,), dtype=torch.float16, device=dev).normal_()
    dst = torch.empty_like(src)
    for _ in range(2):
        dst.copy_(src)
    rate = 2 * src.numel() * 2 / statistics.median(timed_us(lambda: dst.copy_(src), 5) for _ in range(3)) / 1e6     # TB/s
    del src, dst
    torch.cuda.empty_cache()
    say(f"# {torch.cuda.get_device_name(0)}; copy rate measured here: {rate:.2f} TB/s (512 MiB fp16 copy, bytes read + written)")
    gen = torch.Generator(device=dev).manual_seed(0)

    def per_call(name, T, rps, r, distinct):
        """-> one report line: rows form and prompt form of one call, captured, in alternation."""
        K, N, ends = SHAPES[name]
        S, R, slots = T // rps, len(ends) * r, max(distinct, 8)
        iters = max(2, min(a.iters, (1 << 16) // T))
        x = torch.randint(-128, 128, (T, K), device=dev, generator=gen, dtype=torch.int8)
        x_scale = (torch.rand((T,), device=dev, generator=gen) * 0.04 + 0.01).half()
        out = torch.randn((T, N), device=dev, generator=gen).half()
        A = (torch.randn((slots, R, K), device=dev, generator=gen) * 0.02).half()
        B = (torch.randn((slots, N, r), device=dev, generator=gen) * 0.02).half()
        scaling = torch.full((slots,), 2.0, device=dev)
        ws = torch.empty((loramod.workspace_bytes(T, K, r, len(ends)),), dtype=torch.uint8, device=dev)
        ids = (torch.arange(S, device=dev, dtype=torch.int32) * 7 + 3) % distinct
        graphs = {}
        for form in ("rows", "prompt"):
            for _ in range(2):
                loramod.lora_rows(out, x, x_scale, A, B, scaling, ids, rps, ends, workspace=ws, form=form)
            torch.cuda.synchronize()
            graphs[form] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[form]):
                for _ in range(iters):
                    loramod.lora_rows(out, x, x_scale, A, B, scaling, ids, rps, ends, workspace=ws, form=form)
        figs = {form: [] for form in graphs}
        for _ in range(a.reps):
            for form, g in graphs.items():
                out.normal_()                                  # (the in-place sums must not run away over many calls)
                g.replay()
                figs[form].append(timed_us(g.replay, 3) / iters)
        nbytes = min(distinct, S) * (R * K + N * r) * 2 + T * (K + 2 + 4 * N) + 2 * ((K + 511) // 512) * T * R * 4
        ratio = statistics.median(figs["prompt"]) / statistics.median(figs["rows"])
        spread = max((max(v) - min(v)) / statistics.median(v) for v in figs.values())
        from qserve_amd._lib import lib
        planned = loramod.FORMS[lib.qs_lora_rows_form_for_rank(loramod.FORMS.index(loramod.rows_form(T, rps, slots)), r)]
        return (f"    T={T:<6d} rows_per_seq={rps:<5d} {name:8s} r={r:<3d} {distinct:2d} adapters   rows {fig(figs['rows'])}   prompt {fig(figs['prompt'])}   "
                f"prompt / rows {ratio:5.2f} (spread {spread:4.2f})   floor {nbytes / rate / 1e6:7.1f} us   planner: {planned}")

    say(f"# 1. per call: up to {a.iters} calls captured in one hipGraph, HIP events around 3 replays, mean us per call; {a.reps} figures per form in "
        f"alternation, median (lowest .. highest); spread = the larger (highest - lowest) / median of the two forms")
    for T in (4096, 16384):
        for name in SHAPES:
            for rps in SWEEP:
                say(per_call(name, T, rps, 16, 8))
            torch.cuda.empty_cache()
    say("\n# 2. r = 64, and 64 distinct adapters (T = 16 384, rows_per_seq = 256)")
    for name in ("qkv", "gate_up"):
        say(per_call(name, 16384, 256, 64, 8))
        say(per_call(name, 16384, 256, 16, 64))
        torch.cuda.empty_cache()

    if not a.skip_engine:
        from qserve_amd.decode import LLAMA3_8B, DecodeEngine
        slots, rank = 8, 16
        real = loramod.rows_form
        forms = {"planner": real, "rows": lambda *_: "rows"}
        eng = DecodeEngine(LLAMA3_8B, batch=BATCH, prompt_len=PROMPT, max_new=MAX_NEW, device="cuda:0", seed=0)
        prompt = torch.randint(0, LLAMA3_8B["vocab"], (BATCH * PROMPT,), device=dev, generator=torch.Generator(device=dev).manual_seed(1))

        def clocked_ms(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        say(f"\n# 3. {LLAMA3_8B['name']} shapes, KV4: prefill_chunked of {BATCH} x {PROMPT} tokens in chunks of {CHUNK}, eager; host clock + synchronise, ms; "
            f"{a.reps} figures per setting in alternation after one warm-up round (the planner's form for a chunk: {real(BATCH * CHUNK, CHUNK, slots)})")
        off = [clocked_ms(lambda: eng.prefill_chunked(PROMPT, CHUNK, prompt)) for _ in range(a.reps + 1)][1:]
        say(f"    prefill_chunked, LoRA off                 {fig(off, 'ms')}")
        eng.enable_lora(slots, rank)
        g2 = torch.Generator(device=dev).manual_seed(3)
        for layer in eng.lora_table.layers:                   # (random slots written directly: what load() would leave)
            for A, B in layer.values():
                A.copy_((torch.randn(A.shape, device=dev, generator=g2) * 0.01).half())
                B.copy_((torch.randn(B.shape, device=dev, generator=g2) * 0.01).half())
        eng.lora_table.scaling.fill_(2.0)
        for what, ids in (("ids -1", [-1] * BATCH), ("8 adapters", [b % slots for b in range(BATCH)])):
            eng.set_lora(ids)
            t = {name: [] for name in forms}
            for i in range(a.reps + 1):
                for name, f in forms.items():
                    loramod.rows_form = f
                    ms = clocked_ms(lambda: eng.prefill_chunked(PROMPT, CHUNK, prompt))
                    if i:                                         # (the first round warms every shape up)
                        t[name].append(ms)
            for name, v in t.items():
                say(f"    prefill_chunked, {what:10s} form {name:8s} {fig(v, 'ms')}   - off: {statistics.median(v) - statistics.median(off):+8.1f} ms")
        say(f"\n# 4. a {NODES}-node verify_tree (a binary tree) at B = {BATCH} behind that prompt, eight adapters, eager; host clock + synchronise, ms "
            f"(the planner's form: {real(BATCH * NODES, NODES, slots)})")
        parents = [-1] + [(i - 1) // 2 for i in range(1, NODES)]
        draft = torch.randint(0, LLAMA3_8B["vocab"], (BATCH, NODES), device=dev, generator=torch.Generator(device=dev).manual_seed(2))
        t = {name: [] for name in forms}
        for i in range(a.reps + 1):
            for name, f in forms.items():
                loramod.rows_form = f
                ms = clocked_ms(lambda: eng.verify_tree(draft, parents))
                if i:
                    t[name].append(ms)
        loramod.rows_form = real
        for name, v in t.items():
            say(f"    verify_tree, form {name:8s} {fig(v, 'ms')}")


if __name__ == "__main__":
    main()
