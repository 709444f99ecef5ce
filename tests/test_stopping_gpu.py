"""GPU tests of stopping in the engine (DecodeEngine.set_stopping / generate): the text of a sequence is the text of an engine without
stopping, cut by the numpy rule of tests/_stop_cases.py, and nothing of another sequence changes; finished sequences are frozen - state,
text and page slots; capture and generate against eager twins (in processes of their own).  Setting and helpers of
tests/_stop_engine.py."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_step_stops_where_the_rule_cuts_the_twins_text(gpu):
    """Eight step()s of an unstopped twin give the texts.  The table: what sequence 0 emits at step 3 as a single id, what sequence 1
    emits at steps 4 - 5 as a two-token sequence; sequence 2 may generate 6 tokens.  The rule decides where every sequence ends (a
    chosen id may stop another sequence earlier).  After every step the stopping engine holds the twin's text of that step cut by the
    rule; finished sequences stay as they are, pages included."""
    import _accept_engine as E
    import _speculate_engine as S
    import _stop_engine as T
    toks = E.prompt(gpu)
    twin = S.drafting_engine(toks)
    texts = [T.texts_of(twin)]
    for _ in range(8):
        twin.step()
        texts.append(T.texts_of(twin))
    full = texts[-1]
    stop = [full[0][E.P + 3], full[1][E.P + 4:E.P + 6]]
    new = [40, 40, 6]
    e = T.stopping_engine(toks, stop, new)
    watch = T.Frozen(e)
    watch.look("set_stopping")
    for rnd in range(1, 9):
        e.step()
        T.assert_cut_of(e, texts[rnd], stop, new, f"step {rnd}")
        watch.look(f"step {rnd}")
    want = T.assert_cut_of(e, full, stop, new, "after 8 steps")
    assert e.lengths.tolist() == [L for L, _ in want] and e.finished.tolist() == [r for _, r in want]
    assert all(r != 0 for _, r in want), f"the setting left a sequence live: {want}"
    assert want[0][0] <= E.P + 4 and want[1][0] <= E.P + 6 and want[2][0] <= E.P + 6     # (none later than the table and the limit say)
    assert watch.checked() == [0, 1, 2], "a finished sequence was not watched over two frozen steps"


def _speculate_round_by_round(gpu, sampled):
    import _accept_engine as E
    import _penalty_engine as PE
    import _speculate_engine as S
    import _stop_engine as T
    toks = E.prompt(gpu)
    twin, e, ref = (S.drafting_engine(toks) for _ in range(3))
    if sampled:
        for x in (twin, e, ref):
            x.set_sampling(0.8, 50, 0.9, seed=3)
            x.set_penalties(**PE.PLANTED)
    cols = S.plant(ref, (twin, e))                                           # [root, g1 .. g4] per sequence, where the drafter finds it
    stop, new = [int(cols[0, 2])], [40, 4, 40]                               # g2 of sequence 0; sequence 1's limit falls at g3
    e.set_stopping(stop, new)
    watch = T.Frozen(e)
    watch.look("set_stopping")
    for rnd in range(4):
        got = e.speculate(E.PAR, sampled=sampled)
        free = twin.speculate(E.PAR, sampled=sampled)
        want = T.assert_cut_of(e, T.texts_of(twin), stop, new, f"round {rnd}")
        watch.look(f"round {rnd}")
        print(f"round {rnd}: accepted {got[1].tolist()}, unstopped {free[1].tolist()}, finished {e.finished.tolist()}")
        if rnd == 0 and not sampled:
            assert int(free[1][0]) >= 3, "the planted continuation was not accepted: no clip inside a path"
            assert int(got[1][0]) == 2 < int(free[1][0]) and want[0] == (E.P + 3, 1), "sequence 0 was not clipped at g2, inside its path"
        # sequence 2 runs free: bit for bit the unstopped twin's
        assert want[2][1] == 0, "the setting stopped sequence 2"
        assert torch.equal(e.tokens[2], twin.tokens[2]) and torch.equal(e.lengths[2], twin.lengths[2])
        assert torch.equal(e.history[2], twin.history[2]) and torch.equal(got[1][2], free[1][2])
        assert torch.equal(T.slot_bytes(e, 2, int(e.lengths[2]) - 1), T.slot_bytes(twin, 2, int(twin.lengths[2]) - 1))
    # (the sampled texts are other texts: there the rule alone says where sequences 0 and 1 end - the chosen id may come earlier)
    assert sampled or (want[1] == (E.P + 4, 2) and e.finished.tolist()[:2] == [1, 2]), "sequence 1 was not cut at g3 by its limit"
    assert want[0][1] != 0 and want[1][1] != 0
    return watch


def test_speculate_clips_inside_an_accepted_path(gpu):
    watch = _speculate_round_by_round(gpu, sampled=False)
    assert watch.checked() == [0, 1]


def test_sampled_penalised_speculate_is_cut_the_same_way(gpu):
    _speculate_round_by_round(gpu, sampled=True)


def test_switched_off_is_never_switched_on(gpu):
    """set_stopping(...) followed by set_stopping(None) leaves an engine that equals one that never called it: state and pools after
    steps and a speculate round."""
    import _accept_engine as E
    import _speculate_engine as S
    toks = E.prompt(gpu)
    a, b = S.drafting_engine(toks), S.drafting_engine(toks)
    a.set_stopping([int(a.tokens[0]), [1, 2, 3]], 2)
    assert a.finished.tolist() == [1, 0, 0]
    a.set_stopping(None)
    for what in ("step 1", "step 2"):
        a.step()
        b.step()
        E.assert_same_state(a, b, what)
    ra, rb = a.speculate(E.PAR), b.speculate(E.PAR)
    E.assert_same_result(ra, rb, "speculate")
    E.assert_same_state(a, b, "speculate")
    S.assert_same_text(a, b, "speculate")
    assert torch.equal(a.history, b.history) and a._len_bound == b._len_bound


def test_first_token_stop_and_refusals(gpu):
    """The prefill token of sequence 1 in the table: finished by set_stopping itself, and the next step() leaves the sequence untouched
    while the others go on.  Prefill entries and the host walk refuse while stopping is on; limits beyond the history are refused."""
    import _accept_engine as E
    import _speculate_engine as S
    toks = E.prompt(gpu)
    e, free = S.drafting_engine(toks), S.drafting_engine(toks)
    with pytest.raises(AssertionError, match="enable_drafting first"):
        E.engine(toks).set_stopping([1])
    with pytest.raises(AssertionError, match="capacity"):
        e.set_stopping([1], 41)
    first = int(e.tokens[1])
    e.set_stopping([first])
    assert e.finished.tolist() == [0, 1, 0] and e.limit_lens.tolist() == [E.P + 40] * 3
    row = e.history[1].clone()
    e.step()
    free.step()
    assert e.finished.tolist() == [0, 1, 0] and e.lengths.tolist() == [E.P + 2, E.P + 1, E.P + 2]
    assert int(e.tokens[1]) == first and torch.equal(e.history[1], row)
    for b in (0, 2):
        assert torch.equal(e.tokens[b], free.tokens[b]) and torch.equal(e.history[b], free.history[b])
    with pytest.raises(AssertionError, match="set_stopping"):
        e.prefill(E.P, toks)
    with pytest.raises(AssertionError, match="device_walk=True"):
        e.verify_tree(torch.zeros((E.B, len(E.PAR)), dtype=torch.int64, device=gpu), E.PAR)
    with pytest.raises(AssertionError, match="set_stopping first"):
        free.generate(4)
    e.set_stopping([], 1)                                                    # one token each: all at their limit at once
    assert e.finished.tolist() == [2, 2, 2]


def _program(mode, marker):
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tests", "_stop_engine.py"), mode], cwd=ROOT,
                       capture_output=True, text=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and marker in r.stdout, f"exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"


def test_capture_with_stopping_replays_against_an_eager_twin(gpu):
    """tests/_stop_engine.py `capture` in a fresh process under a time limit of its own: capture() and capture_speculate() with stopping
    on, replays against an eager twin in state, text and finish reasons, and a stop table refilled under the captured graph."""
    _program("capture", "STOP-CAPTURE-OK")


def test_generate_polls_every_few_rounds(gpu):
    """tests/_stop_engine.py `generate` in a fresh process (it captures): generate() over steps and over speculation ends with every
    sequence finished before max_rounds, after ceil(rounds / poll_every) read-backs, with the unstopped twins' texts cut by the rule;
    without room in the page tables it returns instead of asserting."""
    _program("generate", "STOP-GENERATE-OK")
