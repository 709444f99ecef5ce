"""Engines with penalties on, and the case a verification's inputs form for tests/_penalty_cases.py, shared by the engine tests of
tests/test_penalize_rows_gpu.py - and, run as a program, the body of its capture test: capture_speculate with penalties on, replays
against an eager twin, new values through set_penalties after the capture, and a captured step().  The capture test starts this file in a
fresh Python process because a failed capture leaves the HIP context unusable and nothing else may share it.

Setting of tests/_speculate_engine.py: TINY, B = 3, P = 70, seed 5, the 12-node tree PAR, n-gram drafting with a planted continuation."""
import os
import sys

import numpy as np
import torch

import _accept_engine as E
import _speculate_engine as S

VALUES = dict(repetition=1.3, frequency=0.2, presence=0.5)
OTHER = dict(repetition=0.7, frequency=1.0, presence=-3.0)
# the capture test plants the continuation of a reference engine into the PROMPT part of the histories: with a neutral repetition the
# plant changes no count that matters (frequency and presence count generated tokens only), so the continuation stays the greedy one
PLANTED = dict(repetition=1.0, frequency=0.2, presence=0.5)


def penalised_engine(toks, values=VALUES):
    e = S.drafting_engine(toks)
    e.set_penalties(**values)
    return e


def case_of(logits, history, lengths, prompt_len, draft, parents, values):
    """The inputs of one penalised head as a case of tests/_penalty_cases.py: `logits` [B, n, V] (unpenalised), the text and the lengths
    from before the head ran, the draft (None: a decode step, n = 1)."""
    B, n, V = logits.shape
    return dict(n=V, n_nodes=n, cap=history.size(1), history=history.cpu().numpy().astype(np.int32), lengths=lengths.cpu().numpy().astype(np.int32),
                prompt_lens=np.full((B,), prompt_len, np.int32), node_tokens=None if draft is None else draft.cpu().numpy(),
                parents=None if draft is None else list(parents), rep=values["repetition"], freq=values["frequency"],
                pres=values["presence"], logits=logits.reshape(B * n, V).cpu().numpy())


def main():
    """capture_speculate with penalties on (its warm-up is a real round) against an eager twin; the continuation planted behind it and
    two replays; then new values through set_penalties on both - the replay follows them, and a twin that kept the old values does
    not agree any more; then a captured step(), which penalises too."""
    gpu = torch.device("cuda:0")
    toks = E.prompt(gpu)
    cap, twin, ref, old = (penalised_engine(toks, PLANTED) for _ in range(4))
    cap.capture_speculate(E.PAR)
    for e in (twin, ref, old):
        e.speculate(E.PAR)
    E.assert_same_state(cap, twin, "after capture_speculate")
    S.assert_same_text(cap, twin, "after capture_speculate")
    S.plant(ref, (cap, twin, old))                           # the PENALISED greedy continuation: ref's step() penalises too
    for i in range(2):
        got = cap.run_speculate()
        want = twin.speculate(E.PAR)
        old.speculate(E.PAR)
        torch.cuda.synchronize()
        E.assert_same_result(got, want, f"replay {i}")
        E.assert_same_state(cap, twin, f"replay {i}")
        S.assert_same_text(cap, twin, f"replay {i}")
        print(f"replay {i}: accepted path lengths {got[1].tolist()}")
        if i == 0:
            assert int(got[1].max()) >= 2, "the planted continuation was accepted nowhere: the replay checked root-only paths"
    # new values after the capture: the graph reads the same device tensors.  `old` keeps the old ones and falls behind.
    E.assert_same_state(old, twin, "the twin that keeps the old values, before they change")
    for e in (cap, twin):
        e.set_penalties(**OTHER)
    got = cap.run_speculate()
    want = twin.speculate(E.PAR)
    old.speculate(E.PAR)
    torch.cuda.synchronize()
    E.assert_same_result(got, want, "replay with new values")
    E.assert_same_state(cap, twin, "replay with new values")
    S.assert_same_text(cap, twin, "replay with new values")
    assert not torch.equal(old.last_verify_logits.view(torch.int16), twin.last_verify_logits.view(torch.int16)), \
        "new values changed nothing: the round with the old values produced the same penalised logits"
    print(f"replay with new values: accepted path lengths {got[1].tolist()}")
    cap.capture()                                            # (its warm-up is a real step)
    twin.step()
    cap.run()
    twin.step()
    E.assert_same_state(cap, twin, "captured step() after the replays")
    S.assert_same_text(cap, twin, "captured step() after the replays")
    for e in (cap, twin):
        e.set_penalties(**VALUES)
    cap.run()
    twin.step()
    E.assert_same_state(cap, twin, "captured step() with new values")
    S.assert_same_text(cap, twin, "captured step() with new values")
    print("PENALTY-CAPTURE-OK")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    main()
