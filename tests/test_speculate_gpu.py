"""GPU tests of the closed speculative loop (DecodeEngine.enable_drafting / draft_tree / speculate / capture_speculate /
run_speculate): an engine that drafts, verifies, commits and records on the device against a twin whose drafter and history append
are the numpy reference of tests/_draft_cases.py - bit-identical results, state and text -, step()'s recording, and the captured
round against an eager twin (in a process of its own).  Setting and helpers of tests/_accept_engine.py."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_speculate_is_draft_verify_append_of_a_numpy_twin(gpu):
    """Engine A calls speculate(PAR); twin B drafts with the numpy reference from its own history, verifies with
    verify_tree(device_walk=True) and appends with numpy.  The greedy continuation is planted in both histories, so round 1 accepts
    more than the root somewhere.  Then two more rounds on the now ragged lengths, and a step() on both."""
    import _accept_engine as E
    import _speculate_engine as S
    toks = E.prompt(gpu)
    a, b = S.drafting_engine(toks), S.drafting_engine(toks)
    assert a.history.dtype == torch.int32 and tuple(a.history.shape) == (E.B, a.max_len)
    assert torch.equal(a.history[:, :E.P], toks.view(E.B, E.P).to(torch.int32)) and torch.equal(a.history[:, E.P], a.tokens.to(torch.int32))
    S.plant(E.engine(toks), (a, b))
    for rnd in range(3):
        len0 = b.lengths.clone()
        tree = a.draft_tree(E.PAR)
        got = a.speculate(E.PAR)
        draft, want = S.numpy_round(b)
        assert tree.dtype == torch.int64 and torch.equal(tree.cpu(), torch.from_numpy(draft)), f"round {rnd}: draft_tree differs"
        E.assert_same_result(got, want, f"round {rnd}")
        E.assert_same_state(a, b, f"round {rnd}")
        assert torch.equal(a.history, b.history), f"round {rnd}: histories differ"
        S.assert_same_text(a, b, f"round {rnd}")
        assert torch.equal(a.lengths, len0 + got[1])
        print(f"round {rnd}: accepted path lengths {got[1].tolist()}")
        if rnd == 0:
            assert int(got[1].max()) >= 2, "the planted continuation was accepted nowhere: only root-only paths were compared"
    a.step()
    b.step()
    E.assert_same_state(a, b, "step() after the rounds")
    S.assert_same_text(a, b, "step() after the rounds")
    assert a._len_bound >= int(a.lengths.max())


def test_sampled_speculate_against_the_numpy_twin(gpu):
    """The same twin construction with the sampling head on.  A sampled token is a function of (seed, sequence, position), so four
    step()s of a third sampling engine give the continuation the walk is about to draw; planted like the greedy one, it makes round 0
    accept more than the root somewhere - the sampled walk and a multi-token append together, not root-only paths."""
    import _accept_engine as E
    import _speculate_engine as S
    toks = E.prompt(gpu)
    a, b, ref = S.drafting_engine(toks), S.drafting_engine(toks), E.engine(toks)
    for e in (a, b, ref):
        e.set_sampling(0.8, 50, 0.9, seed=3)
    S.plant(ref, (a, b))
    for rnd in range(2):
        got = a.speculate(E.PAR, sampled=True)
        _, want = S.numpy_round(b, sampled=True)
        E.assert_same_result(got, want, f"sampled round {rnd}")
        E.assert_same_state(a, b, f"sampled round {rnd}")
        assert torch.equal(a.history, b.history), f"sampled round {rnd}: histories differ"
        S.assert_same_text(a, b, f"sampled round {rnd}")
        print(f"sampled round {rnd}: accepted path lengths {got[1].tolist()}")
        if rnd == 0:
            assert int(got[1].max()) >= 2, "the planted sampled continuation was accepted nowhere: only root-only paths were compared"


def test_step_records_its_token_only_with_drafting_enabled(gpu):
    import _accept_engine as E
    import _speculate_engine as S
    toks = E.prompt(gpu)
    plain, e = E.engine(toks), S.drafting_engine(toks)
    assert plain.history is None
    before = e.history.clone()
    for k in range(1, 3):
        plain.step()
        e.step()
        assert torch.equal(e.history[:, E.P + k], e.tokens.to(torch.int32)) and bool((e.lengths == E.P + 1 + k).all())
    E.assert_same_state(plain, e, "drafting changes nothing but the history")
    before[:, E.P + 1:E.P + 3] = e.history[:, E.P + 1:E.P + 3]
    assert torch.equal(e.history, before), "step() wrote more than its token"
    with pytest.raises(AssertionError, match="enable_drafting first"):
        plain.speculate(E.PAR)


def test_enable_drafting_checks_the_pad_token_and_refills_in_place(gpu):
    """The verification embeds pad nodes: a pad outside the vocabulary is refused.  A second call keeps the buffers a captured graph
    may hold and fills them again."""
    import _accept_engine as E
    import _speculate_engine as S
    from qserve_amd.decode import TINY
    toks = E.prompt(gpu)
    e = E.engine(toks)
    for bad in (-1, TINY["vocab"], 1 << 40):
        with pytest.raises(AssertionError, match="pad_token"):
            e.enable_drafting(toks, pad_token=bad)
    assert e.history is None                                 # (declared by the engine, created by the first call that is accepted)
    e.enable_drafting(toks, **S.NGRAM)
    first, where = e.history.clone(), (e.history.data_ptr(), [t.data_ptr() for t in e._step_record])
    e.history.fill_(7)
    e.enable_drafting(toks, max_ngram=3, min_match=2, pad_token=TINY["vocab"] - 1)
    assert (e.history.data_ptr(), [t.data_ptr() for t in e._step_record]) == where and torch.equal(e.history, first)
    assert e._draft_params == (3, 2, TINY["vocab"] - 1)


def test_capture_speculate_replays_against_an_eager_twin(gpu):
    """tests/_speculate_engine.py as a program, in a fresh process under a time limit of its own: capture_speculate, three
    run_speculate replays and a captured step() against an eager twin.  A capture that succeeds is also the proof that no host
    synchronisation is left in the round."""
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tests", "_speculate_engine.py")], cwd=ROOT,
                       capture_output=True, text=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and "SPECULATE-CAPTURE-OK" in r.stdout, f"exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
