"""Sweep of qs_single_query_attention_long against the two ways the parent serves the same call -> profiles/decode_long.txt.

    python scripts/bench_decode_long.py [--out profiles/decode_long.txt] [--quick]

Per point (KV4 / KV8, H = 32, Hkv = 8, B in 1 / 8 / 64, context 1 024 tokens under a 2 048-entry table, 12 352, 32 768, 131 072):
    long S=plan / 1 / 8 / 16 / 32 / 64   the new entry at the planner's count and at forced counts
    valu                                 qs_single_query_attention at the same shape (tables > 192 entries: its VALU kernel)
    append n=1                           append_attention with one new row per sequence through the split planner (no cache write, no RoPE)
    floor                                the K + V bytes of the step (data, scales, zeros) at 6.29 TB/s
Every sequence has pages of its own while both pools fit POOL_CAP bytes; beyond that the table wraps over the pages that fit (still
far more than the caches hold), as tests/_long_cases.py aliases its pages.  Times are device events around `reps` back-to-back calls
(reps sized for a window of about 30 ms, at least 3), after 3 warm-up calls per variant; 5 such windows per variant, reported as
median [min .. max] per call in us.  The GPU's clocks are whatever the machine runs at: the script reads and prints them, and sets
nothing."""
import argparse
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, HKV = 32, 8
POOL_CAP = 6 << 30
FORCED = (1, 8, 16, 32, 64)
HBM = 6.29e12


def pools(B, mb, int4, dev):
    """-> (kv_pointers int64 [B, 2, mb], K pool, V pool): random data bytes, scale 0.01, zero 8 in every slot."""
    dhb = 64 if int4 else 128
    data, pb = HKV * 64 * dhb, HKV * 64 * dhb + HKV * 64 * 4
    nb = min(B * mb, POOL_CAP // (2 * pb))
    out = []
    for _ in range(2):
        p = torch.randint(0, 256, (nb, pb), dtype=torch.uint8, device=dev)
        meta = torch.cat([torch.full((HKV * 64,), 0.01, dtype=torch.float16, device=dev), torch.full((HKV * 64,), 8.0, dtype=torch.float16, device=dev)])
        p[:, data:] = meta.view(torch.uint8)
        out.append(p)
    idx = (torch.arange(B * mb, dtype=torch.int64, device=dev) % nb).view(B, 1, mb)
    kvp = torch.cat([out[0].data_ptr() + idx * pb, out[1].data_ptr() + idx * pb], dim=1).contiguous()
    return kvp, out[0], out[1], nb < B * mb


def timed(fn, rounds=5):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(), fn(), b.record()
    torch.cuda.synchronize()
    reps = max(3, min(400, int(30.0 / max(a.elapsed_time(b), 1e-3))))
    t = []
    for _ in range(rounds):
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        t.append(a.elapsed_time(b) * 1e3 / reps)
    return float(np.median(t)), min(t), max(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_long.txt"))
    ap.add_argument("--quick", action="store_true", help="B = 1 and the two shortest contexts only (a rehearsal)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_decode_long.py measures on the GPU: no device, no numbers"
    from qserve_amd import append as A
    from qserve_amd.long_decode import single_query_attention_long
    from qserve_amd.plan import attention_long_plan, attention_plan
    from qserve_backend import fused_attention as fa
    dev = torch.device("cuda:0")
    lines = [f"# scripts/bench_decode_long.py on {torch.cuda.get_device_name(0)}; us per call, median [min .. max] of 5 windows"]
    try:
        clk = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30).stdout
        lines += ["# clocks (read, not set): " + l.strip() for l in clk.splitlines() if "sclk" in l or "mclk" in l][:4]
    except Exception as e:                                      # noqa: BLE001
        lines.append(f"# clocks: not read ({e})")
    points = [(1024, 2048), (12352, 193), (32768, 512), (131072, 2048)]
    regrets, slower = [], []
    for int4 in (True, False):
        for B in ((1,) if args.quick else (1, 8, 64)):
            for ctx, mb in (points[:2] if args.quick else points):
                kvp, pk, pv, wrapped = pools(B, mb, int4, dev)
                spt = HKV * (64 if int4 else 128)
                new = torch.randn((B, (H + 2 * HKV) * 128), dtype=torch.float16, device=dev)
                q, k, v = [x.reshape(B, -1, 128) for x in new.split([H * 128, HKV * 128, HKV * 128], dim=-1)]
                lengths = torch.full((B,), ctx, dtype=torch.int32, device=dev)
                past, cu_q = lengths - 1, torch.arange(B + 1, dtype=torch.int32, device=dev)
                plan = attention_long_plan(B, H, HKV, mb, int4)
                floor = B * (ctx - 1) * HKV * 2 * ((64 if int4 else 128) + 4) / HBM * 1e6
                res = {}
                for s in (0,) + FORCED:
                    res[s] = timed(lambda s=s: single_query_attention_long(q, k, v, kvp, lengths, spt, ctx, 1e6, int4, num_splits=s))
                assert attention_plan(B, H, HKV, mb, ctx, int4)["family"] == "valu"
                valu = timed(lambda: fa.single_query_attention(q, k, v, kvp, lengths, None, 8192, 64, spt, ctx, 128, 1e6, True, int4, True))
                app = timed(lambda: A.append_attention(new, cu_q, past, kvp, H, HKV, spt, int4, max_seqlen_q=1, max_past=ctx - 1))
                best = min(FORCED, key=lambda s: res[s][0])
                regret = res[0][0] / res[best][0] - 1
                regrets.append(regret)
                tag = f"{'kv4' if int4 else 'kv8'} B={B:<2d} ctx={ctx:<6d} table={mb:<4d}{' wrapped' if wrapped else ''}"
                lines.append(f"{tag}: floor {floor:8.1f} | long S=plan({plan['splits']}) {res[0][0]:8.1f} [{res[0][1]:.1f} .. {res[0][2]:.1f}] | " +
                             " ".join(f"S={s} {res[s][0]:.1f}" for s in FORCED) +
                             f" | best S={best}, regret {100 * regret:.1f} % | valu {valu[0]:8.1f} [{valu[1]:.1f} .. {valu[2]:.1f}] | "
                             f"append n=1 {app[0]:8.1f} [{app[1]:.1f} .. {app[2]:.1f}] | valu / long {valu[0] / res[0][0]:.2f}")
                print(lines[-1], flush=True)
                if res[0][1] > valu[2]:                          # slower beyond both spreads
                    slower.append(tag)
                del kvp, pk, pv
                torch.cuda.empty_cache()
    lines.append(f"# planner regret against the forced best: mean {100 * np.mean(regrets):.1f} %, worst {100 * max(regrets):.1f} %")
    lines.append("# points where the new entry is slower than the VALU entry beyond the spread: " + ("; ".join(slower) if slower else "none"))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
