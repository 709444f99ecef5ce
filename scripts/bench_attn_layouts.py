#!/usr/bin/env python3
"""The default layout of the two users of the flash tile stager (flash_tile.h stage_fp16_tile) against an OLDER build of the
library, in one job: causal prefill at 16 x 1024 and 4 x 8192 tokens (Llama-3-8B heads, packed qkv) and append attention at
past 4096 / n 512 (KV4).  The two libraries alternate, every run in a fresh child process (a process loads ONE library:
QS_AMD_LIBRARY); per run the median of the timed launches in us.

    python scripts/bench_attn_layouts.py --old PATH/libqserve_amd.so [--runs 3] > profiles/attn_layouts.txt
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, HKV, BASE = 32, 8, 5e5


def child():
    sys.path.insert(0, ROOT)
    import torch
    from bench_append import make_cache, timed
    from qserve_amd import append as A
    from qserve_amd.flash import flash_attn_varlen_func
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    res = {}
    for B, L in ((16, 1024), (4, 8192)):
        T = B * L
        qkv = torch.randn((T, (H + 2 * HKV) * 128), dtype=torch.float16, device=dev, generator=gen)
        q, k, v = qkv.split([H * 128, HKV * 128, HKV * 128], dim=-1)
        q, k, v = q.reshape(T, H, 128), k.reshape(T, HKV, 128), v.reshape(T, HKV, 128)
        cu = torch.arange(0, B + 1, dtype=torch.int32, device=dev) * L
        res[f"prefill {B} x {L}"] = timed(lambda: flash_attn_varlen_func(q, k, v, cu, cu, L, L, causal=True), 30, 5)[0]
        del qkv, q, k, v
    B, past, n = 4, 4096, 512
    pools, tab = make_cache(B, past, n, dev, gen)
    qkv = torch.randn((B * n, (H + 2 * HKV) * 128), dtype=torch.float16, device=dev, generator=gen)
    cu_q = torch.arange(0, B + 1, device=dev, dtype=torch.int32) * n
    pl = torch.full((B,), past, dtype=torch.int32, device=dev)
    A.append_rope_update_kv_cache(qkv, cu_q, pl, tab, H, HKV, HKV * 64, BASE, True)
    out = torch.empty((B * n, H, 128), dtype=torch.float16, device=dev)
    res[f"append past {past} n {n}"] = timed(lambda: A.append_attention(qkv, cu_q, pl, tab, H, HKV, HKV * 64, True, max_seqlen_q=n, out=out), 30, 5)[0]
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", help="the library to compare against (an older build with the same ABI)")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child()
    libs = [("new", None)] + ([("old", os.path.abspath(a.old))] if a.old else [])
    runs = {name: [] for name, _ in libs}
    for r in range(a.runs):
        for name, path in (libs if r % 2 == 0 else libs[::-1]):
            env = dict(os.environ)
            env.pop("QS_AMD_LIBRARY", None)
            if path:
                env.update(QS_AMD_LIBRARY=path, QS_AMD_LIBRARY_AB="1")
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True, timeout=300,
                               cwd=os.path.dirname(os.path.abspath(__file__)))
            if p.returncode != 0:
                sys.exit(f"{name} run {r} failed ({p.returncode}):\n{p.stderr[-2000:]}")
            runs[name].append(json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:]))
    import torch
    print(f"# {torch.cuda.get_device_name(0)}; H={H} Hkv={HKV}; per run: median of 30 launches (us), {a.runs} runs per library in "
          "fresh processes, the libraries alternating")
    for case in runs["new"][0]:
        print(case)
        for name, _ in libs:
            ts = [r[case] for r in runs[name]]
            print(f"    {name:4s} runs {'  '.join(f'{t:9.1f}' for t in ts)}   median {statistics.median(ts):9.1f}  spread {min(ts):9.1f} .. {max(ts):9.1f}")
        if a.old:
            mn, mo = statistics.median(r[case] for r in runs["new"]), statistics.median(r[case] for r in runs["old"])
            lo, hi = min(r[case] for r in runs["old"]), max(r[case] for r in runs["old"])
            print(f"    new / old (medians) {mn / mo:6.4f};  new median {'inside' if lo <= mn <= hi else 'below' if mn < lo else 'ABOVE'} the old build's own spread")


if __name__ == "__main__":
    main()
