"""Per-head Q/K RMSNorm (append.qk_norm_rows, csrc/qk_norm_rows.hip) -> profiles/qk_norm.txt.

    python scripts/bench_qk_norm.py [--out profiles/qk_norm.txt] [--quick]

  rows     H = 32, Hkv = 8, 64 / 768 / 8 192 / 16 384 tokens of packed fp16 qkv rows: the kernel against the same rule written with torch
           ops (float32 mean of squares, rsqrt, two fp16 roundings, in place), and against the bytes' floor - the q and k heads read and
           written once, (H + Hkv) * 256 B each way per token, at 6.29 TB/s.  The v heads are not touched and not counted.
  step     the captured bs = 64 step of a Llama-3-8B-shaped config at 1 024 tokens with qk_norm on against off: the price of one more
           launch per layer.
The two sides of a comparison run in ALTERNATION (bench_window_attention.alternate: 7 windows per side of about 30 ms each after 3
warm-up calls), reported as median [min .. max] per call in us.  Not covered: other head counts, padded rows, the prompt paths of the
engine, tensor parallelism.  Nothing is set on the device."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_window_attention import alternate, fmt      # noqa: E402

H, HKV, EPS = 32, 8, 1e-6
PEAK_BYTES_PER_US = 6.29e6                              # 6.29 TB/s


def torch_rule(qkv, w):
    """The rule of qs_qk_norm_rows with torch ops, in place; w fp16 [H + Hkv, 128]: the two vectors, one row per head."""
    x = qkv[:, :(H + HKV) * 128].view(qkv.size(0), H + HKV, 128)
    xf = x.float()
    t = (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + EPS)).half()
    x.copy_(w * t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qk_norm.txt"))
    ap.add_argument("--quick", action="store_true", help="64 and 768 tokens, no engine step (a rehearsal)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_qk_norm.py measures on the GPU: no device, no numbers"
    from qserve_amd import append as A
    from qserve_amd import decode as D
    dev = torch.device("cuda:0")
    lines = [f"# scripts/bench_qk_norm.py on {torch.cuda.get_device_name(0)}; us per call, median [min .. max] of 7 alternating windows",
             "# rows: eager calls through the Python wrapper, back to back between device events, in place on ONE buffer - a window is",
             "#   bounded below by the host's call rate, and the rows of the call before may still sit in the last-level cache: the floor",
             "#   is the HBM's (6.29 TB/s), so kernel / floor below 1 says the rows did not all come from HBM, nothing else.",
             "# not covered: other head counts, padded rows, the engine's prompt paths, tensor parallelism, a cold-cache call."]

    def emit(s):
        lines.append(s)
        print(s, flush=True)

    gen = torch.Generator(device=dev).manual_seed(0)
    wq, wk = ((torch.rand((128,), device=dev, generator=gen) + 0.5).half() for _ in range(2))
    w = torch.cat([wq.expand(H, 128), wk.expand(HKV, 128)]).contiguous()
    for T in ((64, 768) if args.quick else (64, 768, 8192, 16384)):
        qkv = torch.randn((T, (H + 2 * HKV) * 128), device=dev, generator=gen).half()
        a, b = qkv.clone(), qkv.clone()
        A.qk_norm_rows(a, wq, wk, H, HKV, EPS)
        torch_rule(b, w)
        diff = float((a.float() - b.float()).abs().max())
        kern, ref = alternate(lambda: A.qk_norm_rows(qkv, wq, wk, H, HKV, EPS), lambda: torch_rule(qkv, w))
        floor = 2 * T * (H + HKV) * 256 / PEAK_BYTES_PER_US
        emit(f"rows T={T:<6d} slots={T * (H + HKV):<7d}: kernel {fmt(kern)} | torch {fmt(ref)} | torch / kernel {ref[0] / kern[0]:.2f} | "
             f"bytes' floor {floor:.2f} us, kernel / floor {kern[0] / floor:.2f} | max |kernel - torch| on one call {diff:.3e}")
    if args.quick:
        emit("step: not measured (--quick)")
    else:
        engines = []
        for cfg in (dict(D.LLAMA3_8B, qk_norm=True), D.LLAMA3_8B):
            eng = D.DecodeEngine(cfg, batch=64, prompt_len=1024, max_new=128, device="cuda:0")
            eng.prefill_cache(1024)
            eng.capture()
            engines.append(eng)
        on, off = alternate(engines[0].run, engines[1].run)
        emit(f"step Llama-3-8B shape bs=64 at 1 024 tokens, captured: qk_norm on {fmt(on)} | off {fmt(off)} | on / off {on[0] / off[0]:.4f} | "
             f"on - off {(on[0] - off[0]) / D.LLAMA3_8B['layers']:.2f} us per layer")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
