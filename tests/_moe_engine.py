"""Mixture-of-experts engines shared by tests/test_moe_engine_gpu.py - and, run as a program, the body of its capture test, which starts this
file in a fresh Python process because a failed capture leaves the HIP context unusable and nothing else may share it.

Setting of tests/_accept_engine.py / tests/_speculate_engine.py: B = 3, P = 70, seed 5, the 12-node tree PAR - on TINY_MOE (TINY with 4
experts, 2 per token).  The slow twin is the same engine with the `moe.moe_mlp` seam wrapped by `slow_moe_mlp`: the routing call, then
torch indexing, the DENSE public GEMM ops per expert on the gathered rows, silu_and_mul_quant, and a float32 torch combine in the same
order.  Engines are only compared at equal batch size: the router's matmul is not promised row-independent."""
import contextlib
import os
import sys

import torch

import _accept_engine as E
import _speculate_engine as S


def moe_engine(toks, chunk=None, drafting=False, prefill=True, group_size=-1):
    from qserve_amd.decode import TINY_MOE, DecodeEngine
    e = DecodeEngine(TINY_MOE, batch=E.B, prompt_len=E.P, max_new=40, device="cuda:0", seed=5, group_size=group_size)
    if prefill and chunk is None:
        e.prefill(E.P, toks)
    elif prefill:
        e.prefill_chunked(E.P, chunk, toks)
    if drafting:
        e.enable_drafting(toks, **S.NGRAM)
    return e


def slow_moe_mlp(out, x, x_scale, x_sum, logits, k, gate_up, down, bufs):
    """`moe.moe_mlp` composed slowly (reads the routing back: eager only)."""
    from qserve_amd import fused, moe
    from qserve_amd.decode import W4A8Linear
    ids, w, _, _, _ = moe.route(logits, k)
    T, gs = x.size(0), gate_up.group_size
    y = torch.zeros((T, k, down.n), dtype=torch.float16, device=x.device)
    for e in range(gate_up.experts):
        t_idx, j_idx = (ids == e).nonzero(as_tuple=True)            # row-major: ordered by (t, j)
        n = t_idx.numel()
        if n == 0:
            continue
        xe, se = x[t_idx].contiguous(), x_scale[t_idx].contiguous()
        sume = x_sum[t_idx].contiguous() if x_sum is not None else None
        gu = torch.empty((n, gate_up.n), dtype=torch.float16, device=x.device)
        W4A8Linear.from_tensors(gate_up.expert(e), gs)(xe, se, sume, gu)
        q = torch.empty((n, down.k), dtype=torch.int8, device=x.device)
        qs, qsum = torch.empty((n,), dtype=torch.float16, device=x.device), torch.empty((n,), dtype=torch.float16, device=x.device)
        fused.silu_and_mul_quant(q, gu, qs, qsum if gs == -1 else None)
        ye = torch.empty((n, down.n), dtype=torch.float16, device=x.device)
        W4A8Linear.from_tensors(down.expert(e), gs)(q, qs, qsum if gs == -1 else None, ye)
        y[t_idx, j_idx] = ye
    acc = w[:, 0:1] * y[:, 0].float()
    for j in range(1, k):
        acc = acc + w[:, j:j + 1] * y[:, j].float()
    out.copy_(acc.half())
    return out


@contextlib.contextmanager
def seam(fn):
    """Route every `moe.moe_mlp` call of every engine through fn(original, *args) while the block runs."""
    from qserve_amd import moe
    original = moe.moe_mlp
    moe.moe_mlp = lambda *a: fn(original, *a)
    try:
        yield
    finally:
        moe.moe_mlp = original


def slow(call):
    """call() with the slow composition behind the seam."""
    with seam(lambda original, *a: slow_moe_mlp(*a)):
        return call()


def capture_main():
    """capture() then three run()s of the fast engine against three eager steps of the slow twin; one capture_speculate round likewise."""
    gpu = torch.device("cuda:0")
    toks = E.prompt(gpu)
    cap, twin = moe_engine(toks), slow(lambda: moe_engine(toks))
    E.assert_same_state(cap, twin, "prefill")
    cap.capture()                                            # (its warm-up is a real step)
    slow(twin.step)
    E.assert_same_state(cap, twin, "after capture")
    for i in range(3):
        cap.run()
        slow(twin.step)
        E.assert_same_state(cap, twin, f"step replay {i}")
    print(f"step: tokens {cap.tokens.tolist()}")
    cap, twin = moe_engine(toks, drafting=True), slow(lambda: moe_engine(toks, drafting=True))
    cap.capture_speculate(E.PAR)
    slow(lambda: twin.speculate(E.PAR))
    E.assert_same_state(cap, twin, "after capture_speculate")
    got = cap.run_speculate()
    want = slow(lambda: twin.speculate(E.PAR))
    torch.cuda.synchronize()
    E.assert_same_result(got, want, "round replay")
    E.assert_same_state(cap, twin, "round replay")
    S.assert_same_text(cap, twin, "round replay")
    print(f"round replay: accepted path lengths {got[1].tolist()}")
    print("MOE-CAPTURE-OK")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    {"capture": capture_main}[sys.argv[1]]()
