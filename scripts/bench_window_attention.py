"""Sliding-window attention against its un-windowed counterparts -> profiles/window_attention.txt.

    python scripts/bench_window_attention.py [--out profiles/window_attention.txt] [--quick]

  decode   W = 4 096, KV4 / KV8, H = 32, Hkv = 8, B in 1 / 8 / 64, texts of 4 096 / 32 768 / 131 072 tokens: the windowed entry against
           qs_single_query_attention_long over the same tables.  The expectation is that time stops growing with the text once it is
           past W; the ratios are written, not asserted.
  append   n = 512 new tokens, past 8 192 / 32 768, B = 1: window = 4 096 against the un-windowed append (split planner).
  step     the captured bs = 64 Llama-3-8B step at 1 024 tokens with sliding_window = 4 096 against the fused step without it: the
           price of the un-fused attention + quantiser pair.
The two sides of a comparison run in ALTERNATION - window A, window B, A, B, ... - so that clock drift lands on both; a window is
`reps` back-to-back calls between device events (about 30 ms, at least 3 calls), 7 windows per side after 3 warm-up calls, reported
as median [min .. max] per call in us.  A line that could not be measured says so.  Nothing is set on the device."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_decode_long import H, HKV, pools      # noqa: E402

W = 4096


def alternate(fa, fb, rounds=7):
    """-> ((median, min, max) of fa, the same of fb), us per call, measured in alternating windows."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = []
    for fn in (fa, fb):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        a.record(), fn(), b.record()
        torch.cuda.synchronize()
        reps.append(max(3, min(400, int(30.0 / max(a.elapsed_time(b), 1e-3)))))
    t = ([], [])
    for _ in range(rounds):
        for i, fn in enumerate((fa, fb)):
            a.record()
            for _ in range(reps[i]):
                fn()
            b.record()
            torch.cuda.synchronize()
            t[i].append(a.elapsed_time(b) * 1e3 / reps[i])
    return tuple((float(np.median(x)), min(x), max(x)) for x in t)


def fmt(x):
    return f"{x[0]:8.1f} [{x[1]:.1f} .. {x[2]:.1f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_attention.txt"))
    ap.add_argument("--quick", action="store_true", help="B = 1, KV4, no engine step (a rehearsal)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_window_attention.py measures on the GPU: no device, no numbers"
    from qserve_amd import append as A
    from qserve_amd import decode as D
    from qserve_amd.long_decode import single_query_attention_long
    from qserve_amd.plan import attention_long_plan, attention_window_plan
    dev = torch.device("cuda:0")
    lines = [f"# scripts/bench_window_attention.py on {torch.cuda.get_device_name(0)}; us per call, median [min .. max] of 7 alternating windows"]

    def emit(s):
        lines.append(s)
        print(s, flush=True)

    for int4 in ((True,) if args.quick else (True, False)):
        spt = HKV * (64 if int4 else 128)
        for B in ((1,) if args.quick else (1, 8, 64)):
            for ctx in (4096, 32768, 131072):
                mb = ctx // 64 + 1
                kvp, pk, pv, wrapped = pools(B, mb, int4, dev)
                new = torch.randn((B, (H + 2 * HKV) * 128), dtype=torch.float16, device=dev)
                q, k, v = [x.reshape(B, -1, 128) for x in new.split([H * 128, HKV * 128, HKV * 128], dim=-1)]
                lengths = torch.full((B,), ctx, dtype=torch.int32, device=dev)
                win, full = alternate(lambda: single_query_attention_long(q, k, v, kvp, lengths, spt, ctx, 1e6, int4, window=W),
                                      lambda: single_query_attention_long(q, k, v, kvp, lengths, spt, ctx, 1e6, int4))
                emit(f"decode {'kv4' if int4 else 'kv8'} B={B:<2d} text={ctx:<6d} table={mb:<4d}{' wrapped' if wrapped else ''}: "
                     f"window S=plan({attention_window_plan(B, H, HKV, mb, W, int4)['splits']}) {fmt(win)} | "
                     f"long S=plan({attention_long_plan(B, H, HKV, mb, int4)['splits']}) {fmt(full)} | long / window {full[0] / win[0]:.2f}")
                del kvp, pk, pv
                torch.cuda.empty_cache()
        for past in (8192, 32768):
            n, mb = 512, (past + 512) // 64 + 1
            kvp, pk, pv, _ = pools(1, mb, int4, dev)
            qkv = torch.randn((n, (H + 2 * HKV) * 128), dtype=torch.float16, device=dev)
            cu, pl = torch.tensor([0, n], dtype=torch.int32, device=dev), torch.tensor([past], dtype=torch.int32, device=dev)
            win, full = alternate(lambda: A.append_attention(qkv, cu, pl, kvp, H, HKV, spt, int4, max_seqlen_q=n, window=W),
                                  lambda: A.append_attention(qkv, cu, pl, kvp, H, HKV, spt, int4, max_seqlen_q=n, max_past=past))
            emit(f"append {'kv4' if int4 else 'kv8'} B=1 n={n} past={past:<6d}: window {fmt(win)} | un-windowed (split planner) {fmt(full)} | "
                 f"un-windowed / window {full[0] / win[0]:.2f}")
            del kvp, pk, pv
            torch.cuda.empty_cache()
    if args.quick:
        emit("step: not measured (--quick)")
    else:
        engines = []
        for cfg in (dict(D.LLAMA3_8B, sliding_window=W), D.LLAMA3_8B):
            eng = D.DecodeEngine(cfg, batch=64, prompt_len=1024, max_new=64, device="cuda:0")
            eng.prefill_cache(1024)
            eng.capture()
            engines.append(eng)
        win, fused = alternate(engines[0].run, engines[1].run)
        emit(f"step Llama-3-8B bs=64 at 1 024 tokens, captured: sliding_window={W} (un-fused attention + quant) {fmt(win)} | "
             f"fused step {fmt(fused)} | window / fused {win[0] / fused[0]:.3f}")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
