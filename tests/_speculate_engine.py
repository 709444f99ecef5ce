"""Engines with n-gram drafting, the numpy-drafting twin and the planted continuation shared by tests/test_speculate_gpu.py - and,
run as a program, the body of its capture test: capture_speculate, three run_speculate replays and a captured step() against an eager
twin.  The capture test starts this file in a fresh Python process because a failed capture leaves the HIP context unusable
and nothing else may share it.

Setting of tests/_accept_engine.py: TINY, B = 3, P = 70, seed 5, the 12-node tree PAR whose nodes 1, 4, 7, 10 are a chain from the root."""
import os
import sys

import numpy as np
import torch

import _accept_engine as E
from _draft_cases import reference_append, reference_draft_batch

PLANT = 10                                               # history columns 10 .. 14 receive [root, g1 .. g4]
NGRAM = dict(max_ngram=4, min_match=1, pad_token=0)


def drafting_engine(toks):
    e = E.engine(toks)
    e.enable_drafting(toks, **NGRAM)
    return e


def plant(ref, engines):
    """Make acceptance certain: four step()s of `ref` (an engine in the state of `engines`, used up) give the greedy continuation
    g1 .. g4 of the root; [root, g1 .. g4] goes into columns 10 .. 14 of the engines' histories.  Only the drafter reads it - the
    cache is untouched -, and it finds the root there, followed by what the model is about to say."""
    seq = [ref.tokens.clone()]
    for _ in range(4):
        ref.step()
        seq.append(ref.tokens.clone())
    cols = torch.stack(seq, dim=1).to(torch.int32)
    for e in engines:
        e.history[:, PLANT:PLANT + 5] = cols
    return cols


def numpy_round(twin, sampled=False):
    """One speculate() round with the drafter and the append on the host: the numpy reference drafts from the twin's own history,
    verify_tree(device_walk=True) verifies, numpy appends."""
    hist, lens = twin.history.cpu().numpy(), twin.lengths.cpu().numpy()
    draft = reference_draft_batch(hist, lens, E.PAR, NGRAM["max_ngram"], NGRAM["min_match"], NGRAM["pad_token"])
    res = twin.verify_tree(torch.from_numpy(draft).to(twin.dev), E.PAR, device_walk=True, sampled=sampled)
    new = reference_append(hist, lens - 1, draft, res[0].cpu().numpy(), res[1].cpu().numpy(), twin.tokens.cpu().numpy())
    twin.history.copy_(torch.from_numpy(new))
    return draft, res


def assert_same_text(a, b, what):
    """history[s, :lengths[s]] of both engines, and that its last entry is the current token."""
    torch.cuda.synchronize()
    ha, hb, la, lb = a.history.cpu(), b.history.cpu(), a.lengths.cpu().tolist(), b.lengths.cpu().tolist()
    assert la == lb, f"{what}: lengths differ"
    for s, n in enumerate(la):
        assert torch.equal(ha[s, :n], hb[s, :n]), f"{what}: the text of sequence {s} differs"
        assert int(ha[s, n - 1]) == int(a.tokens[s]), f"{what}: the text of sequence {s} does not end in its current token"


def main():
    """capture_speculate (its warm-up is a real round), the continuation planted behind it, three replays against the eager twin's
    speculate(), then a captured step() - which records its token - against the twin's step()."""
    gpu = torch.device("cuda:0")
    toks = E.prompt(gpu)
    cap, twin, ref = drafting_engine(toks), drafting_engine(toks), drafting_engine(toks)
    cap.capture_speculate(E.PAR)
    twin.speculate(E.PAR)
    ref.speculate(E.PAR)
    E.assert_same_state(cap, twin, "after capture_speculate")
    assert_same_text(cap, twin, "after capture_speculate")
    plant(ref, (cap, twin))
    for i in range(3):
        len0 = twin.lengths.clone()
        got = cap.run_speculate()
        want = twin.speculate(E.PAR)
        torch.cuda.synchronize()
        E.assert_same_result(got, want, f"replay {i}")
        E.assert_same_state(cap, twin, f"replay {i}")
        assert_same_text(cap, twin, f"replay {i}")
        assert torch.equal(cap.lengths, len0 + got[1]) and int(got[1].min()) >= 1
        print(f"replay {i}: accepted path lengths {got[1].tolist()}")
        if i == 0:
            assert int(got[1].max()) >= 2, "the planted continuation was accepted nowhere: the replay checked root-only paths"
    cap.capture()                                            # (its warm-up is a real step)
    twin.step()
    cap.run()
    twin.step()
    E.assert_same_state(cap, twin, "captured step() after the replays")
    assert_same_text(cap, twin, "captured step() after the replays")
    print("SPECULATE-CAPTURE-OK")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    main()
