"""The grouped form of the LoRA row update (`lora.lora_rows(form="grouped")`, csrc/lora_rows.hip) against the rows form, in ONE run
(no pass / fail threshold; figures only - csrc/lora_plan.h takes its constants from the "S sweep" section):

  1. per call, rows form and grouped form in alternation, on the four linears of a Llama-3-8B layer (qkv 4096 -> 6144 in three
     segments, o 4096 -> 4096, gate_up 4096 -> 28672 in two, down 14336 -> 4096), r = 16 and 64, with 1 / 8 / 64 distinct adapters
     (at 64 every group of a decode step is one row: reported, not planned on - the planner cannot see the ids), at T = 64
     (rows_per_seq = 1, a decode step) and T = 768 (rows_per_seq = 12, a tree verification); beside each the time the call's bytes
     would take at the copy rate measured in the same run (distinct adapters' A and B, x, x_scale, out read and written, the float32
     partial planes written and read);
  2. the S sweep: rows_per_seq = 1, S = 64 .. 16 384 sequences, r = 16, 8 adapters (and 64), qkv and gate_up;
  3. the captured Llama-3-8B step at B = 64 (KV4, prompt 1 024) with eight r = 16 adapters and with every id -1, and
  4. an admit of 8 ragged prompts of about 1 024 tokens (passes of 256) under eight adapters, eager, host clock -
     both with the planner's form and with `lora.rows_form` answering "rows" in alternation (the step also with "grouped" forced).
     The rows form's kernels and launcher are those of the commit before the grouped form existed, so "rows" stands for that
     commit here.

Parts 1 and 2: --iters calls captured in one hipGraph after warm-up calls of the same shape, HIP events around three replays; --reps
such figures per form in alternation: median (lowest .. highest).  Run it under `timeout`.

    python scripts/bench_lora_grouped.py [--iters 20] [--reps 3] [--replays 50] [--skip-engine] [--out profiles/lora_grouped.txt]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = dict(qkv=(4096, 6144, (4096, 5120, 6144)), o=(4096, 4096, (4096,)), gate_up=(4096, 28672, (14336, 28672)), down=(14336, 4096, (4096,)))
SWEEP = (64, 256, 1024, 4096, 16384)
PROMPT, BATCH, MAX_NEW = 1024, 64, 640


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--skip-engine", action="store_true", help="parts 1 and 2 only (no 8B engine)")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    assert a.reps >= 3 and torch.cuda.is_available(), "bench_lora_grouped needs a GPU and at least three figures per variant"
    from qserve_amd import lora as loramod
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def timed_us(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n

    def fig(v):
        return f"{statistics.median(v):9.1f} us ({min(v):.1f} .. {max(v):.1f})"

    src = torch.empty((1 << 28,), dtype=torch.float16, device=dev).normal_()
    dst = torch.empty_like(src)
    for _ in range(2):
        dst.copy_(src)
    rate = 2 * src.numel() * 2 / statistics.median(timed_us(lambda: dst.copy_(src), 5) for _ in range(3)) / 1e6     # TB/s
    del src, dst
    torch.cuda.empty_cache()
    say(f"# {torch.cuda.get_device_name(0)}; copy rate measured here: {rate:.2f} TB/s (512 MiB fp16 copy, bytes read + written)")
    gen = torch.Generator(device=dev).manual_seed(0)

    def per_call(name, S, rps, r, distinct):
        """-> one report line: rows form and grouped form of one call, captured, in alternation."""
        K, N, ends = SHAPES[name]
        T, R, slots = S * rps, len(ends) * r, max(distinct, 8)
        iters = max(2, min(a.iters, (1 << 16) // T))
        x = torch.randint(-128, 128, (T, K), device=dev, generator=gen, dtype=torch.int8)
        x_scale = (torch.rand((T,), device=dev, generator=gen) * 0.04 + 0.01).half()
        out = torch.randn((T, N), device=dev, generator=gen).half()
        A = (torch.randn((slots, R, K), device=dev, generator=gen) * 0.02).half()
        B = (torch.randn((slots, N, r), device=dev, generator=gen) * 0.02).half()
        scaling = torch.full((slots,), 2.0, device=dev)
        ws = torch.empty((loramod.workspace_bytes(T, K, r, len(ends)),), dtype=torch.uint8, device=dev)
        ids = (torch.arange(S, device=dev, dtype=torch.int32) * 7 + 3) % distinct       # (interleaved: a group's rows are not adjacent)
        graphs = {}
        for form in ("rows", "grouped"):                       # (not loramod.FORMS: the prompt form refuses rows_per_seq < 16)
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
        ratio = statistics.median(figs["grouped"]) / statistics.median(figs["rows"])
        spread = max((max(v) - min(v)) / statistics.median(v) for v in figs.values())
        return (f"    S={S:<6d} rows_per_seq={rps:<3d} {name:8s} r={r:<3d} {distinct:2d} adapters   rows {fig(figs['rows'])}   grouped {fig(figs['grouped'])}   "
                f"grouped / rows {ratio:5.2f} (spread {spread:4.2f})   floor {nbytes / rate / 1e6:7.1f} us   planner: {loramod.rows_form(T, rps, slots)}")

    say(f"# 1. per call: up to {a.iters} calls captured in one hipGraph, HIP events around 3 replays, mean us per call; {a.reps} figures per form in "
        f"alternation, median (lowest .. highest); spread = the larger (highest - lowest) / median of the two forms")
    for rps in (1, 12):
        for name in SHAPES:
            for r in (16, 64):
                for distinct in (1, 8, 64):
                    say(per_call(name, 64, rps, r, distinct))
    say("\n# 2. S sweep: rows_per_seq = 1, r = 16 (lora_plan.h: GROUPED_MAX_SEQS, GROUPED_MIN_SEQS from the 8-adapter lines)")
    for name in ("qkv", "gate_up"):
        for distinct in (8, 64):
            for S in SWEEP:
                say(per_call(name, S, 1, 16, distinct))
            torch.cuda.empty_cache()

    if not a.skip_engine:
        from qserve_amd.decode import LLAMA3_8B, DecodeEngine
        slots, rank = 8, 16
        real = loramod.rows_form
        forms = {"planner": real, "rows": lambda *_: "rows"}
        eng = DecodeEngine(LLAMA3_8B, batch=BATCH, prompt_len=PROMPT, max_new=MAX_NEW, device="cuda:0", seed=0)
        eng.enable_lora(slots, rank)
        g2 = torch.Generator(device=dev).manual_seed(3)
        for layer in eng.lora_table.layers:                   # (random slots written directly: what load() would leave)
            for A, B in layer.values():
                A.copy_((torch.randn(A.shape, device=dev, generator=g2) * 0.01).half())
                B.copy_((torch.randn(B.shape, device=dev, generator=g2) * 0.01).half())
        eng.lora_table.scaling.fill_(2.0)
        # ---- 4. (first: it leaves the state the step starts from) the admit
        say(f"\n# 4. admit of 8 ragged prompts (1 024 - 17 i tokens) into rows 0 .. 7 of a B = {BATCH} engine, passes of 256, eight r = {rank} adapters, eager; "
            f"host clock + synchronise, ms; {a.reps} figures per form in alternation (the planner's form for {8 * 256} one-row sequences: "
            f"{real(8 * 256, 1, slots)})")
        prompts = [torch.randint(0, LLAMA3_8B["vocab"], (PROMPT - 17 * i,), generator=torch.Generator().manual_seed(i)) for i in range(8)]
        eng.set_lora([b % slots for b in range(BATCH)])
        eng.enable_drafting(None)
        ad = {name: [] for name in forms}
        for i in range(a.reps + 1):
            for name, f in forms.items():
                loramod.rows_form = f
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                eng.admit(list(range(8)), prompts, chunk=256)
                torch.cuda.synchronize()
                if i:                                             # (the first round warms every shape up)
                    ad[name].append((time.perf_counter() - t0) * 1e3)
        for name, t in ad.items():
            say(f"    admit, form {name:8s} {statistics.median(t):9.1f} ms ({min(t):.1f} .. {max(t):.1f})")
        # ---- 3. the captured step
        say(f"\n# 3. {LLAMA3_8B['name']} shapes, KV4, B = {BATCH}, prompt {PROMPT}: the captured step() with {slots} adapters of r = {rank} over the batch and "
            f"with every id -1, LoRA off beside them; host clock around {a.replays} replays + device synchronise, us per replay; 5 figures per "
            f"graph in alternation (the planner's form for the step: {real(BATCH, 1, slots)})")
        prompt = torch.randint(0, LLAMA3_8B["vocab"], (BATCH * PROMPT,), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        eng.set_lora(None)
        eng.prefill_chunked(PROMPT, 256, prompt)
        state0 = (eng.tokens.clone(), eng.lengths.clone(), eng.hidden.clone())
        forms["grouped"] = lambda *_: "grouped"
        settings = {"off": (None, real)}
        for what, ids in (("8 adapters", [b % slots for b in range(BATCH)]), ("ids -1", [-1] * BATCH)):
            settings.update({f"{what}, {name}": (ids, f) for name, f in forms.items()})

        def reset(name):
            eng.tokens.copy_(state0[0])
            eng.lengths.copy_(state0[1])
            eng.hidden.copy_(state0[2])
            eng._len_bound = PROMPT + 1
            if settings[name][0] is not None:
                eng.set_lora(settings[name][0])               # (the graphs share `lora_ids`: refilled in place for the one about to run)

        graphs = {}
        for name, (ids, f) in settings.items():
            loramod.rows_form = f
            eng.set_lora(ids)
            reset(name)
            eng.capture()
            graphs[name] = eng.graph
        loramod.rows_form = real

        def per_replay_us(name):
            reset(name)
            for _ in range(3):
                graphs[name].replay()
            reset(name)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.replays):
                graphs[name].replay()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e6 / a.replays

        figs = {name: [] for name in graphs}
        for _ in range(5):
            for name in graphs:
                figs[name].append(per_replay_us(name))
        for name, t in figs.items():
            d = [y - x for x, y in zip(figs["off"], t)]
            say(f"    captured step, LoRA {name:20s} {fig(t)}   - off: median of pairs {statistics.median(d):+8.1f} us ({min(d):+.1f} .. {max(d):+.1f})")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
