"""Engines, drafts and state comparison shared by the engine tests of tests/test_tree_accept_gpu.py - and, run as a program, the body
of its capture test: capture_verify, then two run_verify calls, against an eager device-walk twin.  The capture test starts this file
in a fresh Python process because a failed capture leaves the HIP context unusable and nothing else may share it.

Setting of tests/test_append_tree_gpu.py::test_engine_verify_tree: TINY, B = 3, P = 70, seed 5, the 12-node tree whose nodes 1, 4, 7, 10
hold the greedy continuation of a reference engine and whose other nodes are siblings that never hold the greedy token."""
import os
import sys

import numpy as np
import torch

B, P = 3, 70
PAR = [-1, 0, 0, 0, 1, 1, 2, 4, 4, 5, 7, 7]
CHAIN = [1, 4, 7, 10]


def prompt(gpu):
    from qserve_amd.decode import TINY
    return torch.randint(0, TINY["vocab"], (B * P,), device=gpu, generator=torch.Generator(device=gpu).manual_seed(1))


def engine(toks):
    from qserve_amd.decode import TINY, DecodeEngine
    e = DecodeEngine(TINY, batch=B, prompt_len=P, max_new=40, device="cuda:0", seed=5)
    e.prefill(P, toks)
    return e


def greedy_draft(ref, rng, gpu):
    """A [B, 12] draft for the state `ref` is in: four step()s of `ref` (which is used up) give g_1 .. g_4 for the chain; the other
    nodes are random, and a sibling of a chain node never holds the greedy token too."""
    from qserve_amd.decode import TINY
    V, n = TINY["vocab"], len(PAR)
    g = []
    for _ in range(4):
        ref.step()
        g.append(ref.tokens.clone())
    draft = torch.from_numpy(rng.integers(0, V, size=(B, n))).to(gpu)
    for k, node in enumerate(CHAIN):
        draft[:, node] = g[k]
        for sib in [c for c in range(n) if PAR[c] == PAR[node] and c != node]:
            draft[:, sib] = (g[k] + 1 + sib) % V
    return draft


def random_draft(rng, gpu):
    from qserve_amd.decode import TINY
    return torch.from_numpy(rng.integers(0, TINY["vocab"], size=(B, len(PAR)))).to(gpu)


def assert_same_result(a, b, what):
    for name, x, y in zip(("accept_idx", "accept_lens", "argmax"), a, b):
        assert x.dtype == y.dtype and torch.equal(x, y), f"{what}: {name} differs"


def assert_same_state(a, b, what):
    """tokens, lengths, hidden and every layer's K and V pools, byte for byte."""
    torch.cuda.synchronize()
    assert torch.equal(a.tokens, b.tokens), f"{what}: tokens differ"
    assert torch.equal(a.lengths, b.lengths), f"{what}: lengths differ"
    assert torch.equal(a.hidden.view(torch.int16), b.hidden.view(torch.int16)), f"{what}: hidden differs"
    for li, ((ka, va), (kb, vb)) in enumerate(zip(a.pools, b.pools)):
        assert torch.equal(ka, kb), f"{what}: layer {li} K pool differs"
        assert torch.equal(va, vb), f"{what}: layer {li} V pool differs"


def main():
    """capture_verify, two replays with different drafts (the first holds the greedy continuation, so paths are longer than the
    root), against a twin that runs the same calls eagerly."""
    gpu = torch.device("cuda:0")
    toks = prompt(gpu)
    rng = np.random.default_rng(3)
    n = len(PAR)
    cap, twin = engine(toks), engine(toks)
    cap.capture_verify(PAR)                                  # its warm-up is a real verification of an all-zero draft
    twin.verify_tree(torch.zeros((B, n), dtype=torch.int64, device=gpu), PAR, device_walk=True)
    assert_same_state(cap, twin, "after capture_verify")
    # a reference in the same state provides the greedy continuation from here
    ref = engine(toks)
    ref.verify_tree(torch.zeros((B, n), dtype=torch.int64, device=gpu), PAR)
    assert_same_state(ref, twin, "host-path reference")
    drafts = [greedy_draft(ref, rng, gpu), random_draft(rng, gpu)]
    for i, d in enumerate(drafts):
        len0 = twin.lengths.clone()
        got = cap.run_verify(d)
        want = twin.verify_tree(d, PAR, device_walk=True)
        torch.cuda.synchronize()
        assert_same_result(got, want, f"replay {i}")
        assert_same_state(cap, twin, f"replay {i}")
        assert torch.equal(cap.lengths, len0 + got[1]) and int(got[1].min()) >= 1
        print(f"replay {i}: accepted path lengths {got[1].tolist()}")
        if i == 0:
            assert int(got[1].max()) >= 2, "the greedy continuation was accepted nowhere: the replay checked root-only paths"
    cap.step()
    twin.step()
    assert_same_state(cap, twin, "step() after the replays")
    print("CAPTURE-OK")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    main()
