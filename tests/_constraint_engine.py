"""Engines under a token automaton shared by tests/test_constraint_engine_gpu.py - and, run as a program, the bodies of its capture
and generate tests, which start this file in a fresh Python process because a failed capture leaves the HIP context unusable
 and nothing else may share it.

Setting of tests/_accept_engine.py / tests/_speculate_engine.py: TINY (vocabulary 512), B = 3, P = 70, seed 5, the 12-node tree PAR.
The automaton: class = token % 7, five states, next[s, c] = (s + c) % 5 where (s + c) % 3 != 0 and -1 elsewhere - every state allows
at least four and refuses at least two of the seven classes.  Sequence 1 is unconstrained (-1)."""
import os
import sys

import numpy as np
import torch

import _accept_engine as E
import _speculate_engine as S
from _constraint_cases import DEAD, move

V, C, STATES = 512, 7, 5
STARTS = [0, -1, 2]


def tables():
    token_class = (np.arange(V) % C).astype(np.int16)
    nxt = np.array([[(s + c) % STATES if (s + c) % 3 else -1 for c in range(C)] for s in range(STATES)], dtype=np.int32)
    return token_class, nxt


def automaton():
    from qserve_amd.constraints import TokenDFA
    token_class, nxt = tables()
    return TokenDFA(torch.from_numpy(token_class), torch.from_numpy(nxt))


def fresh_engine(toks, dfa, starts=STARTS, sampling=None):
    """An engine whose FIRST token is already drawn under the automaton: set_constraint, then prefill, then drafting."""
    from qserve_amd.decode import TINY, DecodeEngine
    e = DecodeEngine(TINY, batch=E.B, prompt_len=E.P, max_new=40, device="cuda:0", seed=5)
    if sampling is not None:
        e.set_sampling(*sampling[0], **sampling[1])
    e.set_constraint(dfa, starts)
    e.prefill(E.P, toks)                                     # (refuses nothing: the constraint needs no history)
    e.enable_drafting(toks, **S.NGRAM)
    return e


def host_moves(states, tokens):
    """Per sequence: is the token allowed in the tracked state (unconstrained: yes), and the state behind it."""
    token_class, nxt = tables()
    out, ok = [], []
    for st, t in zip(states, tokens):
        new = move(int(st), int(t), token_class, nxt, C)
        ok.append(new != DEAD or int(st) == DEAD)
        out.append(new)
    return ok, out


def capture_main():
    """capture_speculate with the constraint on (its warm-up is a real round), a planted continuation, three replays against the eager
    twin - state, text, result and fsm_state -, then new start states filled in place under the captured graph and one more replay."""
    gpu = torch.device("cuda:0")
    toks = E.prompt(gpu)
    dfa = automaton()
    cap, twin, ref = (fresh_engine(toks, dfa) for _ in range(3))
    cap.capture_speculate(E.PAR)
    twin.speculate(E.PAR)
    ref.speculate(E.PAR)
    E.assert_same_state(cap, twin, "after capture_speculate")
    assert torch.equal(cap.fsm_state, twin.fsm_state)
    S.plant(ref, (cap, twin))                                # (ref is constrained too: what it says next is what the twins will say)
    graph, longest = cap.speculate_graph, 0
    for i in range(4):
        if i == 3:                                           # the same automaton, new states: no re-capture, the graph reads them
            for e in (cap, twin):
                e.set_constraint(dfa, [3, 1, -1])
            made = cap._speculate_capture
            assert cap.speculate_graph is graph and made.state["automaton"] is dfa and made.keep[1]["constraint"][0] is cap._fsm
        got = cap.run_speculate()
        want = twin.speculate(E.PAR)
        torch.cuda.synchronize()
        E.assert_same_result(got, want, f"replay {i}")
        E.assert_same_state(cap, twin, f"replay {i}")
        S.assert_same_text(cap, twin, f"replay {i}")
        assert torch.equal(cap.fsm_state, twin.fsm_state), f"replay {i}: fsm_state differs"
        longest = max(longest, int(got[1].max()))
        print(f"replay {i}: accepted path lengths {got[1].tolist()}, fsm_state {cap.fsm_state.tolist()}")
    assert longest >= 2, "the planted continuation was accepted nowhere: the replays checked root-only paths"
    assert DEAD not in cap.fsm_state.tolist()
    print("CONSTRAINT-CAPTURE-OK")


def generate_main():
    """generate() under an automaton that forces exactly four tokens of class 3 and then only eos, with eos as the stop token: every
    text is four tokens plus eos, every reason is 1 (a stop sequence) and every state ends in the sink.  Then the constraint is
    switched off and generate() must not replay the graph that masks."""
    from qserve_amd.constraints import TokenDFA
    gpu = torch.device("cuda:0")
    toks = E.prompt(gpu)
    eos, sink = V - 1, 5
    token_class = (np.arange(V) % C).astype(np.int16)
    token_class[eos] = C                                     # a class of its own: C + 1 classes
    nxt = np.full((6, C + 1), -1, dtype=np.int32)
    for s in range(4):
        nxt[s, 3] = s + 1
    nxt[4, C] = nxt[sink, C] = sink
    dfa = TokenDFA(torch.from_numpy(token_class), torch.from_numpy(nxt))
    e = fresh_engine(toks, dfa, starts=0)                    # the prefill ran with the constraint on and drew token 1 of 4
    assert e.fsm_state.tolist() == [1, 1, 1]
    e.set_stopping(stop=[eos])
    texts, reasons, rounds, reads = e.generate(16, poll_every=2)
    print(f"texts {texts}, reasons {reasons}, rounds {rounds}, read-backs {reads}")
    for t in texts:
        assert len(t) == 5 and all(x % C == 3 and x != eos for x in t[:4]) and t[4] == eos, t
    assert reasons == [1, 1, 1] and e.fsm_state.tolist() == [sink] * 3 and rounds <= 6
    with_mask = e.graph
    assert e._step_capture.state["automaton"] is dfa and e._step_capture.keep[1]["constraint"][0] is e._fsm
    e.set_constraint(None)
    e.set_stopping([], [8, 8, 8])
    e.generate(2, poll_every=2)
    assert e.graph is not with_mask, "generate replayed a step graph that still masks"
    print("CONSTRAINT-GENERATE-OK")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    {"capture": capture_main, "generate": generate_main}[sys.argv[1]]()
