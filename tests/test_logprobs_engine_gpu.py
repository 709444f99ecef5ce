"""DecodeEngine.set_logprobs on the GPU, on the TINY engines of tests/_accept_engine.py / tests/_speculate_engine.py (B = 3): the logs
against the float64 oracle of tests/_logprob_cases.py evaluated on the very logits the heads produced, round by round; an engine with
log-probabilities on against a twin without; clipped paths and frozen rows; logprobs() against generate()'s texts.  The capture cases
run tests/_logprob_engine.py in a fresh process."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("tempered", [False, True])
def test_steps_record_the_oracles_values_and_change_nothing_else(gpu, tempered):
    """Six eager step()s (with `tempered`: the sampling head at T = 0.8, penalties on - the logs describe the penalised logits): after
    each, column lengths[b] of the logs holds the oracle's values for the new token on the step's logits, every other entry is
    unchanged, and tokens, lengths, text and pages equal those of a twin that never heard of set_logprobs."""
    import _accept_engine as E
    import _logprob_engine as LP
    import _speculate_engine as S
    from _logprob_cases import slots
    toks = E.prompt(gpu)
    on, twin = LP.tap(S.drafting_engine(toks)), S.drafting_engine(toks)
    if tempered:
        for e in (on, twin):
            e.set_sampling(*LP.SAMPLING[0], **LP.SAMPLING[1])
            e.set_penalties(1.3, 0.2, 0.1)
    top = 5
    on.set_logprobs(top=top, tempered=tempered)
    assert tuple(on.logprob_log.shape) == (E.B, LP.CAP) and on.logprob_log.dtype == torch.float32
    assert tuple(on.rank_log.shape) == (E.B, LP.CAP) and on.rank_log.dtype == torch.int32
    assert tuple(on.top_ids_log.shape) == (E.B, LP.CAP, top) and tuple(on.top_lp_log.shape) == (E.B, LP.CAP, top)
    first = LP.logs_of(on)
    assert np.isnan(first[0]).all() and (first[1] == 0).all() and (first[2] == -1).all() and np.isnan(first[3]).all()
    for i in range(6):
        before, L = LP.logs_of(on), LP.np_(on.lengths)
        on.step()
        twin.step()
        E.assert_same_state(on, twin, f"step {i}")
        S.assert_same_text(on, twin, f"step {i}")
        written = slots(None, None, None, LP.np_(on.tokens), L, E.B, 1, 1, LP.CAP)
        assert [(s[0], s[4]) for s in written] == [(b, int(L[b])) for b in range(E.B)]
        LP.assert_round(before, LP.logs_of(on), on.seen_logits, written, 0.8 if tempered else 1.0, top, f"step {i}")
    if not tempered:                                         # a greedy head: every token is the first of its row's order
        after = LP.logs_of(on)
        assert (after[1][:, E.P + 1:E.P + 7] == 1).all()
        assert np.array_equal(after[2][:, E.P + 1:E.P + 7, 0], LP.np_(on.history)[:, E.P + 1:E.P + 7])


def test_speculate_rounds_record_the_accepted_path(gpu):
    """Four speculate() rounds over a planted continuation: the kernel gathers the rows on the accepted path from `last_verify_logits`
    and scores each for the token behind it - the oracle's slot rule on (draft, accept_idx, accept_lens, tokens) -, nothing else
    changes, and the twin without log-probabilities ends in the same state."""
    import _accept_engine as E
    import _logprob_engine as LP
    import _speculate_engine as S
    from _logprob_cases import slots
    toks = E.prompt(gpu)
    on, twin, ref = (S.drafting_engine(toks) for _ in range(3))
    top, n = 3, len(E.PAR)
    on.set_logprobs(top=top)
    S.plant(ref, (on, twin))
    longest = 0
    for i in range(4):
        before, L = LP.logs_of(on), LP.np_(on.lengths)
        draft = LP.np_(on.draft_tree(E.PAR))
        got = on.speculate(E.PAR)
        want = twin.speculate(E.PAR)
        E.assert_same_result(got, want, f"round {i}")
        E.assert_same_state(on, twin, f"round {i}")
        S.assert_same_text(on, twin, f"round {i}")
        m = LP.np_(got[1])
        written = slots(draft, LP.np_(got[0]), m, LP.np_(on.tokens), L, E.B, n, n, LP.CAP)
        assert len(written) == int(m.sum()) and np.array_equal(LP.np_(on.lengths), L + m)
        hit = LP.assert_round(before, LP.logs_of(on), on.last_verify_logits.reshape(E.B * n, -1), written, 1.0, top, f"round {i}")
        for b in range(E.B):                                 # the round's columns are the round's text positions
            assert np.nonzero(hit[b])[0].tolist() == list(range(int(L[b]), int(L[b] + m[b])))
        longest = max(longest, int(m.max()))
    assert longest >= 3, "no round accepted a path of three nodes: the gather was only checked near the root"
    after, lens = LP.logs_of(on), on.lengths.cpu().tolist()
    hist = LP.np_(on.history)
    for b, Lb in enumerate(lens):                            # greedy verification: every emitted token is its row's first
        assert (after[1][b, E.P + 1:Lb] == 1).all() and np.array_equal(after[2][b, E.P + 1:Lb, 0], hist[b, E.P + 1:Lb])
    with pytest.raises(AssertionError, match="device_walk=True"):
        on.verify_tree(torch.zeros((E.B, n), dtype=torch.int64, device=gpu), E.PAR)


def test_a_clipped_path_records_k_columns_and_a_frozen_row_none(gpu):
    """A stop id inside the planted continuation of sequence 0: the round's path is clipped to k tokens, exactly k columns are written
    - with the oracle's values for the clipped path - and from the next round on the frozen row writes nothing."""
    import _accept_engine as E
    import _logprob_engine as LP
    import _speculate_engine as S
    from _logprob_cases import slots
    toks = E.prompt(gpu)
    on, free, ref = (S.drafting_engine(toks) for _ in range(3))
    top, n = 2, len(E.PAR)
    cols = S.plant(ref, (on, free)).cpu().tolist()
    j0 = max((j for j in (1, 2, 3) if cols[0][j] not in cols[0][:j]), default=None)
    assert j0 is not None, f"the setting gives no token to stop at: sequence 0 continues {cols[0]}"
    on.set_stopping([cols[0][j0]])
    on.set_logprobs(top=top)
    unclipped = LP.np_(free.speculate(E.PAR)[1])
    before, L = LP.logs_of(on), LP.np_(on.lengths)
    draft = LP.np_(on.draft_tree(E.PAR))
    got = on.speculate(E.PAR)
    k = LP.np_(got[1])
    assert k[0] == j0 < unclipped[0] and int(on.finished[0]) == 1, f"sequence 0: k = {k[0]}, unclipped {unclipped[0]}, stop at e_{j0}"
    written = slots(draft, LP.np_(got[0]), k, LP.np_(on.tokens), L, E.B, n, n, LP.CAP)
    assert len(written) == int(k.sum())
    hit = LP.assert_round(before, LP.logs_of(on), on.last_verify_logits.reshape(E.B * n, -1), written, 1.0, top, "the clipped round")
    assert np.nonzero(hit[0])[0].tolist() == list(range(int(L[0]), int(L[0]) + j0))
    for i in range(2):                                       # frozen: k = 0, no column
        before = LP.logs_of(on)
        got = on.speculate(E.PAR) if i == 0 else None
        if i == 1:
            on.step()
        after = LP.logs_of(on)
        for old, new in zip(before, after):
            assert np.array_equal(LP.bits(old)[0], LP.bits(new)[0]), "the frozen sequence 0 wrote a log entry"
        if i == 0:
            assert int(got[1][0]) == 0
    live = [b for b in range(E.B) if int(on.finished[b]) == 0]
    lens = on.lengths.cpu().tolist()
    lp = LP.logs_of(on)[0]
    for b in live:                                           # the live rows' step did record: their text is covered to its end
        assert np.isfinite(lp[b, E.P + 1:lens[b]]).all() and np.isnan(lp[b, lens[b]:]).all()
    assert np.isnan(lp[0, lens[0]:]).all()


def test_prefill_records_the_first_token_and_logprobs_reads_the_text(gpu):
    """set_logprobs before the prefill: the prefill head's token lands at column P.  logprobs() returns the entries of positions
    P .. lengths - 1, one per generated token; set_logprobs(None) stops the recording, and a second on-call clears the logs."""
    import _accept_engine as E
    import _logprob_engine as LP
    from _logprob_cases import slots
    from qserve_amd.decode import TINY, DecodeEngine
    toks = E.prompt(gpu)
    e = LP.tap(DecodeEngine(TINY, batch=E.B, prompt_len=E.P, max_new=40, device="cuda:0", seed=5))
    with pytest.raises(AssertionError, match="set_sampling first"):
        e.set_logprobs(top=1, tempered=True)
    with pytest.raises(AssertionError, match="top=33"):
        e.set_logprobs(top=33)
    e.set_logprobs(top=4)
    before = LP.logs_of(e)
    e.prefill(E.P, toks)
    written = slots(None, None, None, LP.np_(e.tokens), np.full(E.B, E.P), E.B, 1, 1, LP.CAP)
    LP.assert_round(before, LP.logs_of(e), e.seen_logits, written, 1.0, 4, "prefill")
    assert e.lengths.tolist() == [E.P + 1] * E.B
    for _ in range(3):
        e.step()
    e.set_logprobs(None)
    e.step()                                                 # not recorded
    out = e.logprobs()
    logs = LP.logs_of(e)
    for b, o in enumerate(out):
        assert len(o["logprobs"]) == len(o["ranks"]) == len(o["top_ids"]) == len(o["top_logprobs"]) == 5
        assert np.array_equal(np.asarray(o["logprobs"], dtype=np.float32), logs[0][b, E.P:E.P + 5], equal_nan=True)
        assert np.isfinite(o["logprobs"][:4]).all() and np.isnan(o["logprobs"][4]) and o["ranks"] == [1, 1, 1, 1, 0]
        assert all(len(ids) == 4 for ids in o["top_ids"]) and o["top_ids"][4] == [-1] * 4
    e.set_logprobs(top=4)                                    # the same tensors, cleared
    assert np.isnan(LP.logs_of(e)[0]).all()
    e.set_logprobs(top=0)                                    # another width: new tensors, no lists
    assert tuple(e.top_ids_log.shape) == (E.B, LP.CAP, 0)
    e.step()
    assert np.isfinite(LP.logs_of(e)[0][:, E.P + 5]).all() and (LP.logs_of(e)[1][:, E.P + 5] == 1).all()


def _program(mode, marker):
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tests", "_logprob_engine.py"), mode], cwd=ROOT,
                       capture_output=True, text=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and marker in r.stdout, f"exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"


def test_capture_with_logprobs_replays_against_an_eager_twin(gpu):
    """tests/_logprob_engine.py `capture` in a fresh process under a time limit of its own: capture() and capture_speculate() with
    log-probabilities on (tempered, the sampling head on), replays bit-equal to an eager twin in state, text and all four logs."""
    _program("capture", "LOGPROB-CAPTURE-OK")


def test_generate_recaptures_and_logprobs_align_with_its_texts(gpu):
    """tests/_logprob_engine.py `generate` in a fresh process (it captures): a step graph and a speculate graph captured without the
    launch are captured again, a matching one is kept, and logprobs() has one entry per token of generate()'s texts - rank 1 and the
    token itself at the head of its top list under the greedy head."""
    _program("generate", "LOGPROB-GENERATE-OK")
