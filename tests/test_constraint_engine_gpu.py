"""DecodeEngine.set_constraint on the GPU, on the TINY engines of tests/_constraint_engine.py (B = 3, sequence 1 unconstrained): the
masked rows of a verification against the rule applied to an unconstrained twin's rows, the walk over them, the states against a host
walk of the automaton; constrained step()s token by token; the same under the sampling head.  The capture and generate cases run
tests/_constraint_engine.py in a fresh process."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLING = ((0.8,), dict(top_k=50, top_p=0.9, seed=3))


def test_the_automaton_leaves_every_state_a_choice():
    """Checked on the CPU: every state allows at least two classes (the model keeps a say) and refuses at least one (the mask bites)."""
    import _constraint_engine as CE
    token_class, nxt = CE.tables()
    assert ((nxt >= 0).sum(axis=1) >= 2).all() and ((nxt < 0).sum(axis=1) >= 1).all() and nxt.max() < CE.STATES
    assert sorted(set(token_class.tolist())) == list(range(CE.C))


@pytest.mark.parametrize("sampled", [False, True])
def test_speculate_masks_every_row_with_its_own_nodes_state(gpu, sampled):
    """Twin engines from one seed and one state, the constraint off on A and on on B, one speculate() each: B's last_verify_logits are
    bit-equal to the rule applied to A's under the host-computed node states of A's draft, B's path and bonus token are the walk over
    the head's tokens on those rows (greedy: their arg-max), fsm_state is the host advance, and the unconstrained sequence 1 is
    bit-identical to A's."""
    import _accept_engine as E
    import _constraint_engine as CE
    import _speculate_engine as S
    from _constraint_cases import restate_advance, restate_node_states, restate_rows
    from _sample_cases import walk
    toks = E.prompt(gpu)
    a, b = S.drafting_engine(toks), S.drafting_engine(toks)
    if sampled:
        for e in (a, b):
            e.set_sampling(*SAMPLING[0], **SAMPLING[1])
    b.set_constraint(CE.automaton(), CE.STARTS)
    assert b.fsm_state.tolist() == CE.STARTS and b.fsm_state.dtype == torch.int32
    lens = a.lengths.clone()
    draft = a.draft_tree(E.PAR)
    res_a = a.speculate(E.PAR, sampled=sampled)
    idx, n_acc, am = b.speculate(E.PAR, sampled=sampled)
    torch.cuda.synchronize()
    token_class, nxt = CE.tables()
    n = len(E.PAR)
    draft_h = draft.cpu().numpy()
    states = restate_node_states(np.array(CE.STARTS, dtype=np.int32), draft_h, E.PAR, token_class, nxt, CE.C)
    assert torch.equal(b._fsm_node_state[:E.B * n].view(E.B, n).cpu(), torch.from_numpy(states))
    rows_a = a.last_verify_logits.reshape(E.B * n, -1).cpu().numpy().view(np.uint16)
    got = b.last_verify_logits.reshape(E.B * n, -1).cpu().numpy().view(np.uint16)
    want = restate_rows(rows_a, CE.V, states.reshape(-1), token_class, nxt, CE.C)
    assert np.array_equal(got, want), f"{int((got != want).sum())} masked logits differ from the rule"
    assert int((want != rows_a).sum()) >= n * CE.V // 7, "the mask hardly touched the rows"
    assert np.array_equal(got[n:2 * n], rows_a[n:2 * n]), "the unconstrained sequence's rows changed"
    rows = got.view(np.float16).astype(np.float32).reshape(E.B, n, -1)
    for s in range(E.B):
        heads = am[s].tolist()
        if not sampled:
            assert heads == rows[s].argmax(axis=1).tolist(), f"sequence {s}: the head's tokens"
        for i in range(n):                                             # no head ever yields a token its row's state refuses
            if 0 <= states[s, i] < CE.STATES:
                assert nxt[states[s, i], token_class[heads[i]]] >= 0, f"sequence {s}, node {i}: token {heads[i]} in state {states[s, i]}"
        path, bonus = walk(E.PAR, draft_h[s].tolist(), heads)
        assert idx[s, :int(n_acc[s])].tolist() == path and int(b.tokens[s]) == bonus, f"sequence {s}: the walk"
    want_state = restate_advance(np.array(CE.STARTS, dtype=np.int32), states, idx.cpu().numpy(), n_acc.cpu().numpy(), b.tokens.cpu().numpy(),
                                 token_class, nxt, CE.C, max_accept=n)
    assert b.fsm_state.tolist() == want_state.tolist() and CE.DEAD not in want_state.tolist()
    assert want_state[1] == -1 and (want_state[[0, 2]] >= 0).all()
    assert torch.equal(b.lengths, lens + n_acc)
    assert int(b.tokens[1]) == int(a.tokens[1]) and torch.equal(res_a[0][1], idx[1]) and torch.equal(res_a[2][1], am[1])


@pytest.mark.parametrize("sampled", [False, True])
def test_constrained_steps_emit_only_what_the_automaton_allows(gpu, sampled):
    """An engine whose prefill already ran under the constraint, then 12 step()s: every emitted token - the prefill's first one included -
    is allowed by a host walk of the automaton, fsm_state tracks that walk, no state is ever dead; the masked tokens differ from an
    unconstrained twin's somewhere (the constraint decided something) while the unconstrained sequence says what the twin says."""
    import _accept_engine as E
    import _constraint_engine as CE
    toks = E.prompt(gpu)
    samp = SAMPLING if sampled else None
    e = CE.fresh_engine(toks, CE.automaton(), sampling=samp)
    free = CE.fresh_engine(toks, CE.automaton(), starts=-1, sampling=samp)       # on, every sequence unconstrained
    assert free.fsm_state.tolist() == [-1, -1, -1]
    tracked, differ = list(CE.STARTS), 0
    for i in range(13):
        if i:
            e.step()
            free.step()
        emitted = e.tokens.tolist()
        ok, tracked = CE.host_moves(tracked, emitted)
        assert all(ok), f"token {i}: {emitted} from the states before it - not allowed"
        assert e.fsm_state.tolist() == tracked and CE.DEAD not in tracked, f"token {i}: fsm_state {e.fsm_state.tolist()} != {tracked}"
        assert emitted[1] == int(free.tokens[1]), f"token {i}: the unconstrained sequence changed"
        differ += emitted[0] != int(free.tokens[0]) or emitted[2] != int(free.tokens[2])
    assert differ >= 1, "the constraint never decided a token"
    assert free.fsm_state.tolist() == [-1, -1, -1]


def test_the_host_walk_refuses_and_the_prefill_does_not(gpu):
    import _accept_engine as E
    import _constraint_engine as CE
    toks = E.prompt(gpu)
    e = CE.fresh_engine(toks, CE.automaton())
    with pytest.raises(AssertionError, match="device_walk=True"):
        e.verify_tree(torch.zeros((E.B, len(E.PAR)), dtype=torch.int64, device=gpu), E.PAR)
    from qserve_amd.constraints import TokenDFA
    with pytest.raises(AssertionError, match="names 64 tokens, the vocabulary has 512"):
        e.set_constraint(TokenDFA(torch.zeros(64, dtype=torch.int16), torch.zeros((1, 1), dtype=torch.int32)))
    e.set_constraint(None)
    e.verify_tree(torch.zeros((E.B, len(E.PAR)), dtype=torch.int64, device=gpu), E.PAR)    # off again: the host walk runs


def test_start_states_of_every_integer_kind_and_the_tables_across_off(gpu):
    """start_states as a Python int, a numpy integer, a 0-d tensor, a numpy array and a device tensor fill fsm_state alike; anything
    that is not integers is refused with a message; switching off and on again with the same TokenDFA object keeps the uploaded
    tables (the very tensors a capture made with them reads), another object uploads its own."""
    import numpy as np

    import _accept_engine as E
    import _constraint_engine as CE
    dfa = CE.automaton()
    e = CE.fresh_engine(E.prompt(gpu), dfa)
    state, tables = e.fsm_state, e._fsm
    for starts, want in ((3, [3, 3, 3]), (np.int64(2), [2, 2, 2]), (np.int32(-1), [-1, -1, -1]), (torch.tensor(4), [4, 4, 4]),
                         (np.array([0, -1, 2], dtype=np.int32), [0, -1, 2]), (torch.tensor([1, 2, -1], device=gpu), [1, 2, -1]),
                         ((np.int16(4), 0, -1), [4, 0, -1])):
        e.set_constraint(dfa, starts)
        assert e.fsm_state.tolist() == want and e.fsm_state is state and e._fsm is tables, starts
    for bad in (1.0, [0.0, 1.0, 2.0], [[0, 1, 2]], True):
        with pytest.raises(AssertionError, match="one int, or one int per sequence"):
            e.set_constraint(dfa, bad)
    with pytest.raises(AssertionError, match="one per sequence"):
        e.set_constraint(dfa, [0, 1])
    e.set_constraint(None)
    assert e._fsm is None and e._kept_tensors()["constraint"] is None
    e.set_constraint(dfa, [2, -1, 0])
    assert e._fsm is tables and e.fsm_state is state and e.fsm_state.tolist() == [2, -1, 0]
    e.set_constraint(CE.automaton(), 1)
    assert e._fsm is not tables and e.fsm_state.tolist() == [1, 1, 1]


def _program(mode, marker):
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tests", "_constraint_engine.py"), mode], cwd=ROOT,
                       capture_output=True, text=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and marker in r.stdout, f"exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"


def test_capture_speculate_with_a_constraint_replays_against_an_eager_twin(gpu):
    """tests/_constraint_engine.py `capture` in a fresh process under a time limit of its own: capture_speculate with the constraint on,
    three replays against an eager twin in state, text and fsm_state, then new start states filled in place and one more replay."""
    _program("capture", "CONSTRAINT-CAPTURE-OK")


def test_generate_under_an_automaton_that_counts_to_four(gpu):
    """tests/_constraint_engine.py `generate` in a fresh process (it captures): four tokens of one class, then eos, which stops."""
    _program("generate", "CONSTRAINT-GENERATE-OK")
