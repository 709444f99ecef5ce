"""What per-sequence LoRA adapters cost (`qs_lora_rows`, DecodeEngine.set_lora), in ONE run (no pass / fail threshold; figures only):

  1. the lora_rows call (two launches: shrink + expand) on the four linears of a Llama-3-8B layer - qkv 4096 -> 6144 in three segments,
     o 4096 -> 4096, gate_up 4096 -> 28672 in two segments, down 14336 -> 4096 - at T = 64 rows (a decode step at B = 64, one row per
     sequence) and T = 768 (64 sequences x 12 rows, a tree verification), r in {8, 16, 64}, with 1, 8 and 64 distinct adapters over the
     64 sequences, with 8 adapters and every second sequence at -1, and with every sequence at -1 (both launches leave at once: what
     the launches themselves cost); next to each: the time the bytes the call has to move would take
     at the copy rate measured in the same run (distinct adapters' A and B slices, x, x_scale, out read and written, the float32 partial
     planes written and read), and a torch path on the same rows (index_select of every row's A and B, bmm in fp16 with float32
     accumulation per stage and segment, the add);
  2. the captured Llama-3-8B step at B = 64 (KV4, prompt 1 024) with LoRA off (what the engine launches without this feature), on with
     every id -1 (the unfused path of the four linears, every lora_rows workgroup leaving at once) and on with eight r = 16 adapters
     over the batch, as an in-process A/B: the three graphs replayed in alternation;
  3. prefill_chunked of 64 x 1 024 tokens in chunks of 256 under the same three settings (host clock, eager): what the row kernels
     cost where a segmented MFMA GEMM would be the tool - it is not part of this work.

Part 1: --iters calls captured in one hipGraph after warm-up calls of the same shape (device time: no host work between the
launches), HIP events around three replays, --reps such figures per variant in alternation: median (lowest .. highest); the torch
path runs eagerly between HIP events.  Parts 2 and 3: a host clock around work that ends in a device synchronise.
Run it under `timeout`.

    python scripts/bench_lora_rows.py [--iters 20] [--warmup 3] [--reps 3] [--replays 50] [--skip-step] [--skip-prefill] [--out profiles/lora_rows.txt]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SEQS = 64
SHAPES = (("qkv", 4096, 6144, (4096, 5120, 6144)), ("o", 4096, 4096, (4096,)), ("gate_up", 4096, 28672, (14336, 28672)),
          ("down", 14336, 4096, (4096,)))
ROWS_PER_SEQ = (1, 12)
RANKS = (8, 16, 64)
PATTERNS = (("1 adapter", 1, False), ("8 adapters", 8, False), ("64 adapters", 64, False), ("8 adapters, half at -1", 8, True),
            ("every sequence at -1", 0, False))
PROMPT, BATCH, MAX_NEW = 1024, 64, 640


def torch_path(out, x, x_scale, A, B, scaling, row_adapter, seg_ends, r):
    """The same update with torch ops (rows of an id < 0 masked out): gather, two bmm per segment, add."""
    ok = row_adapter >= 0
    idx = row_adapter.clamp(min=0).long()
    Ag, Bg = torch.index_select(A, 0, idx), torch.index_select(B, 0, idx)
    t = torch.bmm(Ag, x.half().unsqueeze(2)).float().squeeze(2) * x_scale.float().unsqueeze(1)
    sc = (torch.index_select(scaling, 0, idx) * ok).unsqueeze(1)
    n0 = 0
    for g, n1 in enumerate(seg_ends):
        d = torch.bmm(Bg[:, n0:n1].float(), t[:, g * r:(g + 1) * r].unsqueeze(2)).squeeze(2)
        out[:, n0:n1] = (out[:, n0:n1].float() + sc * d).half()
        n0 = n1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--skip-step", action="store_true", help="part 1 only (no 8B engine)")
    ap.add_argument("--skip-prefill", action="store_true", help="no part 3")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    assert a.iters >= 10 and a.reps >= 3 and a.replays >= 10
    assert torch.cuda.is_available(), "bench_lora_rows needs a GPU"
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

    # the yardstick of the floors: a device copy of 1 GiB (read + write), far beyond the caches
    src = torch.empty((1 << 29,), dtype=torch.float16, device=dev).normal_()
    dst = torch.empty_like(src)
    for _ in range(2):
        dst.copy_(src)
    rate = 2 * src.numel() * 2 / statistics.median(timed_us(lambda: dst.copy_(src), 5) for _ in range(3)) / 1e6     # TB/s
    del src, dst
    torch.cuda.empty_cache()
    say(f"# {torch.cuda.get_device_name(0)}; copy rate measured here: {rate:.2f} TB/s (1 GiB fp16 copy, bytes read + written)")
    say(f"# 1. lora_rows on {SEQS} sequences; {a.iters} calls captured in one hipGraph, HIP events around 3 replays, mean us per call; {a.reps} figures per variant "
        f"in alternation, median (lowest .. highest); floor = the call's bytes at the copy rate; torch = index_select + bmm on the same rows")
    gen = torch.Generator(device=dev).manual_seed(0)
    for rps in ROWS_PER_SEQ:
        T = SEQS * rps
        for name, K, N, ends in SHAPES:
            x = torch.randint(-128, 128, (T, K), device=dev, generator=gen, dtype=torch.int8)
            x_scale = (torch.rand((T,), device=dev, generator=gen) * 0.04 + 0.01).half()
            out = torch.randn((T, N), device=dev, generator=gen).half()
            for r in RANKS:
                R = len(ends) * r
                A = (torch.randn((SEQS, R, K), device=dev, generator=gen) * 0.02).half()
                B = (torch.randn((SEQS, N, r), device=dev, generator=gen) * 0.02).half()
                scaling = torch.full((SEQS,), 2.0, device=dev)
                ws = torch.empty((loramod.workspace_bytes(T, K, r, len(ends)),), dtype=torch.uint8, device=dev)
                variants = {}
                for pname, distinct, half in PATTERNS:
                    ids = torch.arange(SEQS, device=dev, dtype=torch.int32) % distinct if distinct else \
                        torch.full((SEQS,), -1, dtype=torch.int32, device=dev)
                    if half:
                        ids[1::2] = -1
                    row_ids = ids.repeat_interleave(rps)
                    active = int((ids >= 0).sum()) * rps
                    used = len(set(ids[ids >= 0].tolist()))
                    nbytes = used * (R * K + N * r) * 2 + active * (K + 2 + 4 * N) + 2 * ((K + 511) // 512) * active * R * 4
                    for _ in range(a.warmup):
                        loramod.lora_rows(out, x, x_scale, A, B, scaling, ids, rps, ends, workspace=ws)
                    torch.cuda.synchronize()
                    g = torch.cuda.CUDAGraph()                             # (a.iters calls in one graph: device time, no host in between)
                    with torch.cuda.graph(g):
                        for _ in range(a.iters):
                            loramod.lora_rows(out, x, x_scale, A, B, scaling, ids, rps, ends, workspace=ws)
                    variants[pname] = (g, row_ids, nbytes / rate / 1e6, ids)      # (ids: the graph reads this tensor)
                figs = {(p, w): [] for p in variants for w in ("hip", "torch")}
                for _ in range(a.reps):
                    for p, (g, row_ids, _, _) in variants.items():
                        g.replay()
                        figs[(p, "hip")].append(timed_us(g.replay, 3) / a.iters)
                        out.normal_()                                      # (the in-place sums must not run away over thousands of calls)
                        ref = lambda: torch_path(out, x, x_scale, A, B, scaling, row_ids, ends, r)                          # noqa: E731
                        for _ in range(a.warmup):
                            ref()
                        figs[(p, "torch")].append(timed_us(ref, max(3, a.iters // 4)))
                        out.normal_()
                for p, (_, _, floor, _) in variants.items():
                    h, t = figs[(p, "hip")], figs[(p, "torch")]
                    say(f"    T={T:<4d} {name:8s} r={r:<3d} {p:24s} lora_rows {statistics.median(h):8.1f} us ({min(h):.1f} .. {max(h):.1f})   "
                        f"floor {floor:6.1f} us   torch {statistics.median(t):9.1f} us ({min(t):.1f} .. {max(t):.1f})")
                del A, B, ws, variants
            del x, out
            torch.cuda.empty_cache()

    if not a.skip_step:
        from qserve_amd.decode import LLAMA3_8B, DecodeEngine
        slots, rank = 8, 16
        say(f"\n# 2. {LLAMA3_8B['name']} shapes, KV4, B = {BATCH}, prompt {PROMPT}: the captured step(), LoRA off / on with every id -1 / on with "
            f"{slots} adapters of r = {rank} over the batch; host clock around {a.replays} replays + device synchronise, us per replay; {a.reps} "
            f"figures per graph in alternation")
        prompt = torch.randint(0, LLAMA3_8B["vocab"], (BATCH * PROMPT,), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        eng = DecodeEngine(LLAMA3_8B, batch=BATCH, prompt_len=PROMPT, max_new=MAX_NEW, device="cuda:0", seed=0)
        eng.enable_lora(slots, rank)
        g2 = torch.Generator(device=dev).manual_seed(3)
        for layer in eng.lora_table.layers:                   # (random slots written directly: what load() would leave, without its host loop)
            for A, B in layer.values():
                A.copy_((torch.randn(A.shape, device=dev, generator=g2) * 0.01).half())
                B.copy_((torch.randn(B.shape, device=dev, generator=g2) * 0.01).half())
        eng.lora_table.scaling.fill_(2.0)
        settings = {"off": None, "on, ids -1": [-1] * BATCH, "on, 8 adapters": [b % slots for b in range(BATCH)]}
        if not a.skip_prefill:
            say(f"#    first 3.: prefill_chunked of {BATCH} x {PROMPT} tokens, chunks of 256 (T = {BATCH * 256} rows per pass), eager, host clock + "
                f"synchronise, ms; {a.reps} figures per setting in alternation")
            pf = {name: [] for name in settings}
            for i in range(a.reps + 1):
                for name, ids in settings.items():
                    eng.set_lora(ids)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    eng.prefill_chunked(PROMPT, 256, prompt)
                    torch.cuda.synchronize()
                    if i:                                             # (the first round warms every shape up)
                        pf[name].append((time.perf_counter() - t0) * 1e3)
            for name, t in pf.items():
                d = [y - x for x, y in zip(pf["off"], t)]
                say(f"    prefill_chunked, LoRA {name:16s} {statistics.median(t):9.1f} ms ({min(t):.1f} .. {max(t):.1f})   - off: median of pairs "
                    f"{statistics.median(d):+8.1f} ms")
        eng.set_lora(None)
        eng.prefill_chunked(PROMPT, 256, prompt)
        state0 = (eng.tokens.clone(), eng.lengths.clone(), eng.hidden.clone())

        def reset(name):
            eng.tokens.copy_(state0[0])
            eng.lengths.copy_(state0[1])
            eng.hidden.copy_(state0[2])
            eng._len_bound = PROMPT + 1
            if settings[name] is not None:
                eng.set_lora(settings[name])                  # (the graphs share `lora_ids`: refilled in place for the one about to run)

        graphs = {}
        for name, ids in settings.items():
            eng.set_lora(ids)
            reset(name)
            eng.capture()
            graphs[name] = eng.graph

        def per_replay_us(name):
            g = graphs[name]
            reset(name)
            for _ in range(3):
                g.replay()
            reset(name)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.replays):
                g.replay()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e6 / a.replays

        figs = {name: [] for name in graphs}
        for _ in range(max(a.reps, 5)):
            for name in graphs:
                figs[name].append(per_replay_us(name))
        for name, t in figs.items():
            d = [y - x for x, y in zip(figs["off"], t)]
            say(f"    captured step, LoRA {name:16s} {statistics.median(t):9.1f} us ({min(t):.1f} .. {max(t):.1f})   - off: median of pairs "
                f"{statistics.median(d):+8.2f} us ({min(d):+.2f} .. {max(d):+.2f})")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
