"""DecodeEngine.fork and admit(copy_rows=) on the GPU against a TWIN that never shares: TINY, B = 3, a pool of 12 pages.  Engine A
runs one prompt pass and forks; the twin admits the same prompt into every row by itself (the launches of A's leader, three times).
Rows are compared with tests/_page_engine.assert_same_rows - tokens, lengths, hidden and every K / V slot below lengths - 1, byte for
byte, read through each engine's own page ids -, so a branch that read or wrote a sibling's page shows.  The helpers of
tests/_page_engine.py / tests/_prefix_engine.py are used read-only."""
import pytest
import torch

import _page_engine as E
import _page_ref_cases as R
from _prefix_engine import page_bytes, tokens

pytestmark = pytest.mark.gpu

B, CAP_P, MAX_NEW, N, CHUNK = 3, 191, 40, 12, 128
SEED = 3          # set_sampling(1.0, seed=SEED): the twin's three rows draw different first tokens (asserted on the twin alone below)


def engine(share, sampling=None, **kw):
    from qserve_amd.decode import TINY, DecodeEngine
    e = DecodeEngine(TINY, batch=B, prompt_len=CAP_P, max_new=MAX_NEW, device="cuda:0", seed=5, **dict(dict(page_pool=N, share_pages=share), **kw))
    e.enable_drafting(None, **E.NGRAM)
    e.set_stopping((), 0)                                                   # every row frozen until it is admitted
    if sampling is not None:
        e.set_sampling(1.0, seed=sampling)
    return e


def admit_pair(X, sampling=None, **kw):
    """(A: X admitted once with rows 1 and 2 as copies, the twin: X admitted into each row by itself)."""
    a, twin = engine(True, sampling), engine(False, sampling)
    a.admit([0], [X], max_new_tokens=MAX_NEW - 2, chunk=CHUNK, copy_rows=[[1, 2]], **kw)
    for r in range(B):
        twin.admit([r], [X], max_new_tokens=MAX_NEW - 2, chunk=CHUNK, **kw)
    return a, twin


def same_texts(a, twin, what):
    E.assert_same_rows(a, twin, what)
    assert torch.equal(a.history, twin.history) and torch.equal(a.finished, twin.finished), what
    assert torch.equal(a.prompt_lens, twin.prompt_lens) and torch.equal(a.limit_lens, twin.limit_lens), what


@pytest.mark.parametrize("P", [128, 129, 150, 191])
def test_copy_rows_are_the_twins_rows(gpu, P):
    a, twin = admit_pair(tokens(P, 1))
    w, t = divmod(P, 64)
    snap = a.pager.snapshot()
    shared = snap["page_ids"][0, :w].tolist()
    assert snap["owned"].tolist() == [w + (t > 0)] * 3 and snap["page_ids"][:, :w].tolist() == [shared] * 3
    assert snap["refs"][shared].tolist() == [3] * w and a.pager.free_pages() == N - (w + 3 * (t > 0))
    assert twin.pager.free_pages() == N - 3 * (w + (t > 0))
    if P == 150:
        assert snap["owned"].tolist() == [3, 3, 3] and a.pager.free_pages() == 7 and twin.pager.free_pages() == 3
    if P == 128:                                                            # nothing to copy: no page popped for the followers
        assert snap["owned"].tolist() == [2, 2, 2] and a.pager.free_pages() == 10
    before = page_bytes(a, shared)
    same_texts(a, twin, f"P={P}, behind the admit")
    for i in range(4):
        a.step(), twin.step()
        same_texts(a, twin, f"P={P}, step {i}")
    snap = a.pager.snapshot()
    last = (P + 4 - 1) // 64                                                 # the page of the last written slot, lengths - 2
    assert snap["owned"].tolist() == [last + 1] * 3
    tails = snap["page_ids"][:, w:last + 1]
    assert len(set(tails.reshape(-1).tolist())) == tails.size              # behind the shared pages every row has its own
    assert all(torch.equal(x, y) for x, y in zip(before, page_bytes(a, shared)))
    assert a.lengths.tolist() == [P + 5] * 3 and a.tokens.tolist() == [int(a.tokens[0])] * 3     # greedy: one text
    R.check_invariant(E.pool_state(a))
    a.check()


def test_sampled_branches_diverge_and_each_is_the_twins_row(gpu):
    """Keys follow the row: under a sampler the three branches are the twin's three rows bit for bit, and they differ from each other -
    so every branch wrote its own K / V into its own copy of the tail page (P = 150: 22 shared slots in it) and read it back."""
    a, twin = admit_pair(tokens(150, 1), sampling=SEED)
    same_texts(a, twin, "behind the admit")
    for i in range(8):
        a.step(), twin.step()
        same_texts(a, twin, f"step {i}")
    texts = [twin.history[r, 150:159].tolist() for r in range(B)]
    assert len({tuple(t) for t in texts}) >= 2, f"seed {SEED}: the twin's rows drew one text {texts[0]} - pick another seed"
    assert [a.history[r, 150:159].tolist() for r in range(B)] == texts
    R.check_invariant(E.pool_state(a))
    a.check()


@pytest.mark.parametrize("k", [0, 3])
def test_fork_in_the_middle_of_a_text(gpu, k):
    """P = 125: lengths 126 behind the admit; k = 3 steps put lengths - 1 on the page boundary 128 (two whole pages, nothing copied)."""
    X = tokens(125, 4)
    a, twin = engine(True), engine(False)
    a.admit([0], [X], max_new_tokens=MAX_NEW - 2, chunk=CHUNK)
    for r in range(B):
        twin.admit([r], [X], max_new_tokens=MAX_NEW - 2, chunk=CHUNK)
    for _ in range(k):
        a.step(), twin.step()
    a.fork(0, [2, 1])
    w, t = divmod(125 + k, 64)
    snap = a.pager.snapshot()
    shared = snap["page_ids"][0, :w].tolist()
    assert snap["owned"].tolist() == [snap["owned"][0], w + (t > 0), w + (t > 0)] and snap["refs"][shared].tolist() == [3] * w
    before = page_bytes(a, shared)
    same_texts(a, twin, f"k={k}, behind the fork")
    for i in range(4):
        a.step(), twin.step()
        same_texts(a, twin, f"k={k}, step {i}")
    for i in range(2):                                                      # trees: nodes and commit_path stay behind lengths - 1
        a.speculate(E.PAR), twin.speculate(E.PAR)
        same_texts(a, twin, f"k={k}, round {i}")
    assert all(torch.equal(x, y) for x, y in zip(before, page_bytes(a, shared)))
    R.check_invariant(E.pool_state(a))
    a.check()


def test_stopping_penalties_a_constraint_and_logprobs_ride_along(gpu):
    import _constraint_engine as C
    X = tokens(150, 6)
    a, twin = engine(True), engine(False)
    for e in (a, twin):
        e.set_stopping([[int(X[3])]], 0)
        e.set_penalties(repetition=1.3, frequency=0.1, presence=0.1)
        e.set_constraint(C.automaton(), -1)
        e.set_logprobs(2)
    a.admit([0], [X], max_new_tokens=9, start_states=2, chunk=CHUNK)
    for r in range(B):
        twin.admit([r], [X], max_new_tokens=9, start_states=2, chunk=CHUNK)
    for _ in range(2):
        a.step(), twin.step()
    a.fork(0, [1, 2])
    for i in range(4):
        same_texts(a, twin, f"step {i}")
        assert torch.equal(a.fsm_state, twin.fsm_state) and a.fsm_state.tolist() == [int(a.fsm_state[0])] * 3
        for x, y in zip((a.logprob_log, a.rank_log, a.top_ids_log, a.top_lp_log), (twin.logprob_log, twin.rank_log, twin.top_ids_log, twin.top_lp_log)):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), f"step {i}: a log differs"
        a.step(), twin.step()
    assert len(a.logprobs()[2]["ranks"]) == int(a.lengths[2]) - 150
    a.check()


def test_release_order_and_the_last_page(gpu):
    from qserve_amd import stopping
    a = engine(True, prefix_cache=True)
    a.admit([0], [tokens(150, 1)], max_new_tokens=MAX_NEW - 2, chunk=CHUNK, copy_rows=[[1, 2]])
    ids = a.pager.page_ids.cpu()
    shared = ids[0, :2].tolist()
    before = page_bytes(a, shared)
    a.release_rows([0])                                                     # the source first: the followers keep everything
    a.finished[0], a.lengths[0] = stopping.LENGTH, 1                        # (a harvested row, as serve() leaves it: it takes no page again)
    assert a.pager.refs[shared].tolist() == [3, 3] and a.pager.free_pages() == N - 4
    a.step()
    assert all(torch.equal(x, y) for x, y in zip(before, page_bytes(a, shared))) and a.tokens[1] == a.tokens[2]
    R.check_invariant(E.pool_state(a), cache=shared)
    a.release_rows([1, 2])
    assert a.pager.free_pages() == N - 2 and sorted(a.evict_prefixes(N)) == sorted(shared)
    assert a.pager.free_pages() == N and not a.pager.refs.any()
    R.check_invariant(E.pool_state(a))
    # one free page too few: a pool of 4 pages holds the leader's 3 and ONE copy of the tail page
    b = engine(True, page_pool=4)
    b.admit([0], [tokens(150, 1)], max_new_tokens=MAX_NEW - 2, chunk=CHUNK, copy_rows=[[1, 2]])
    assert b.pager.owned.tolist() == [3, 3, 0] and b.finished.tolist() == [0, 0, stopping.NO_PAGES] and b.pager.free_pages() == 0
    twin = engine(False)
    for r in range(2):
        twin.admit([r], [tokens(150, 1)], max_new_tokens=MAX_NEW - 2, chunk=CHUNK)
    E.assert_same_rows(b, twin, "the served rows", rows=[0, 1])
    R.check_invariant(E.pool_state(b))
    b.check()


def test_refusals(gpu):
    from qserve_amd.decode import TINY, DecodeEngine
    plain = engine(False)
    X = tokens(70, 1)
    plain.admit([0], [X], max_new_tokens=5)
    with pytest.raises(AssertionError, match="counted page pool"):
        plain.fork(0, [1])
    with pytest.raises(AssertionError, match="counted page pool"):
        plain.admit([0], [X], max_new_tokens=5, copy_rows=[[1]])
    with pytest.raises(AssertionError, match="runs on one GPU"):
        DecodeEngine(TINY, batch=B, prompt_len=CAP_P, max_new=MAX_NEW, device="cuda:0", page_pool=N, share_pages=True, tp_rank=0, tp_world=2)
    a = engine(True)
    a.admit([0], [X], max_new_tokens=5)
    for rows in ([0], [1, 1], [B]):
        with pytest.raises(AssertionError, match="distinct row indices"):
            a.fork(0, rows)
    with pytest.raises(AssertionError, match="distinct row indices in 0 .. 2 overall"):
        a.admit([0, 1], [X, X], max_new_tokens=5, copy_rows=[[1], []])
    with pytest.raises(AssertionError, match="asks for n=4 samples - 1 .. batch = 3"):
        a.serve([(X, 4, 4)])
    with pytest.raises(AssertionError, match="counted page pool"):
        plain.serve([(X, 4, 2)])
    assert a.pager.free_pages() == N - 2 and a.pager.owned.tolist() == [2, 0, 0]
    a.check()
