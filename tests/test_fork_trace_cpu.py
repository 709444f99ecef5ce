"""DecodeEngine.fork and admit(copy_rows=) on the host (the recorder and stubs of tests/test_engine_trace_cpu.py, the stand-ins of the
counted page entries of tests/test_page_refs_contracts.py and of the fork entry of tests/test_page_fork_contracts.py, which copies the
pools' bytes): what is launched and in which order, what the rows and the pool look like afterwards, `PrefixCache.row_held`, and the
refusals, which fire before any call."""
import numpy as np
import pytest
import torch

import _page_ref_cases as R


def _engine(monkeypatch, batch=3, **kw):
    import test_page_fork_contracts as FC
    import test_prefix_trace_cpu as PT
    from qserve_amd._lib import SIGNATURES, lib
    D, rec, make = PT._engine(monkeypatch, batch, **dict(dict(prefix_cache=False, share_pages=True), **kw))
    monkeypatch.setattr(lib, "qs_pages_fork", rec.wrap("qs_pages_fork", FC._fake_fork, SIGNATURES["qs_pages_fork"][1]))
    return D, rec, make


def _tokens(n, seed):
    return torch.randint(0, 512, (n,), generator=torch.Generator().manual_seed(seed))


def _state(eng):
    p = eng.pager
    return dict(p.snapshot(), bases=p.layer_bases.numpy(), N=p.N, mb=p.mb, page_bytes=p.page_bytes)


def _same(a, b):
    """Equal, NaN included (the stubbed layers leave NaNs in the activations and the empty log entries are NaN)."""
    return torch.equal(torch.nan_to_num(a.float(), nan=12345.0), torch.nan_to_num(b.float(), nan=12345.0))


def _names(rec, at):
    return [line.split()[0] for line in rec.lines[at:]]


def _ready(make, stopping=True):
    eng = make()
    g = torch.Generator().manual_seed(11)                                   # (the stubs write no K / V: what a copy moves is this)
    for pair in eng.pools:
        for t in pair:
            t.copy_(torch.randint(0, 256, t.shape, generator=g, dtype=torch.uint8))
    eng.enable_drafting(None, max_ngram=3, min_match=1, pad_token=7)
    if stopping:
        eng.set_stopping((), 0)
    return eng


def test_row_held_is_the_inverse_of_row_released():
    from qserve_amd.prefix import PrefixCache
    c = PrefixCache()
    toks = list(range(200))
    assert c.insert(toks, [4, 9, 2]) == [4, 9, 2] and c.evictable() == 0      # the inserting row holds them
    assert c.row_held([4, 9, 7]) == [4, 9]                                   # a second row; page 7 is none of the cache's
    c.row_released([4, 9, 2])
    assert c.evictable() == 1 and c.evict(3) == [2]                         # 4 and 9 are still held by the second row
    c.row_released([4, 9, 7])
    assert c.evictable() == 2 and c.evict(3) == [9, 4] and len(c) == 0
    assert c.row_held([4]) == []


@pytest.mark.parametrize("prefix_cache", [False, True])
def test_admit_with_copy_rows_is_the_leaders_admit_one_fork_and_one_head(built_lib, monkeypatch, prefix_cache):
    D, rec, make = _engine(monkeypatch, prefix_cache=prefix_cache)
    X = _tokens(150, 1)
    with np.errstate(all="ignore"):
        plain = _ready(make)
        at = len(rec.lines)
        plain.admit([0], [X], max_new_tokens=8, chunk=128)
        alone = _names(rec, at)
        eng = _ready(make)
        at = len(rec.lines)
        eng.admit([0], [X], max_new_tokens=8, chunk=128, copy_rows=[[1, 2]])
        grouped = _names(rec, at)
    # release, [the cache's hold behind the passes,] reserve, the leader's passes, ONE fork, ONE head: the leader's list and one entry
    assert grouped.count("pages_fork") == 1 and [n for n in grouped if n != "pages_fork"] == alone
    pages = [n for n in grouped if n.startswith("pages_")]
    assert pages == ["pages_unhold", "pages_reserve_refs"] + ["pages_hold"] * prefix_cache + ["pages_fork"]
    words = rec.lines[at + grouped.index("pages_fork")].split()
    assert words[12] == "finished" and words[13:17] == ["3", str(eng.mb), str(len(eng.layers)), "9"], words
    # admit without copy_rows (and with empty lists) records what it recorded
    with np.errstate(all="ignore"):
        again = _ready(make)
        at = len(rec.lines)
        again.admit([0], [X], max_new_tokens=8, chunk=128, copy_rows=[[]])
    assert _names(rec, at) == alone
    # the rows: one text, one first token (greedy), their own pages behind the two shared ones
    snap = eng.pager.snapshot()
    assert snap["owned"].tolist() == [3, 3, 3] and snap["count"] == 9 - 5 and snap["error"] == 0
    assert snap["page_ids"][:, :2].tolist() == [[0, 1]] * 3 and sorted(snap["page_ids"][:, 2].tolist()) == [2, 3, 4]
    assert snap["refs"].tolist()[:5] == [3 + prefix_cache, 3 + prefix_cache, 1, 1, 1]
    R.check_invariant(_state(eng), cache=[0, 1] if prefix_cache else [])
    k0, v0 = eng.pools[0]
    assert all(torch.equal(k0[snap["page_ids"][r, 2]], k0[snap["page_ids"][0, 2]]) for r in (1, 2)) and bool(k0[2].any())
    assert eng.lengths.tolist() == [151] * 3 and eng.tokens.tolist() == [eng.tokens.tolist()[0]] * 3
    assert eng.prompt_lens.tolist() == [150] * 3 and eng.limit_lens.tolist() == [158] * 3 and eng._text_starts == [150] * 3
    assert torch.equal(eng.history[1], eng.history[0]) and torch.equal(eng.history[2], eng.history[0]) and eng.history[0, 150] == eng.tokens[0]
    assert _same(eng.hidden[2], eng.hidden[0]) and eng.finished.tolist() == [0, 0, 0]
    if prefix_cache:
        assert eng._row_cached == {0: [0, 1], 1: [0, 1], 2: [0, 1]} and eng.prefix.by_page[0].rows == 3
        eng.release_rows([0, 1])
        assert eng.prefix.evictable() == 0                                   # row 2 still holds both cached pages
        eng.release_rows([2])
        assert eng.prefix.evictable() == 2 and sorted(eng.evict_prefixes(9)) == [0, 1]
    else:
        assert eng.prefix is None and eng._row_cached == {}
        eng.release_rows([0])                                               # the source first: the followers' pages stay
        assert eng.pager.refs.tolist()[:5] == [2, 2, 0, 1, 1]
        eng.release_rows([1, 2])
    assert eng.pager.free_pages() == 9 and not eng.pager.refs.any()


def test_fork_copies_the_rows_state_and_launches_release_and_fork(built_lib, monkeypatch):
    D, rec, make = _engine(monkeypatch)
    with np.errstate(all="ignore"):
        eng = _ready(make, stopping=False)
        eng.set_logprobs(2)
        eng.admit([0, 1], [_tokens(70, 1), _tokens(30, 2)])
        eng.step()
        at = len(rec.lines)
        eng.fork(0, [2, 1])
    assert _names(rec, at) == ["pages_unhold", "pages_fork"]
    assert eng.lengths.tolist() == [72, 72, 72] and eng._text_starts == [70, 70, 70]
    for t in eng._row_tensors():
        assert _same(t[1], t[0]) and _same(t[2], t[0]), t.shape
    assert len(eng._row_tensors()) == 10                                    # (no stop rule, no constraint, no adapters)
    snap = eng.pager.snapshot()
    # len - 1 = 71: page 0 shared, page 1 (7 slots written) copied into rows 1 and 2 in row order
    assert snap["owned"].tolist() == [2, 2, 2] and snap["page_ids"][:, 0].tolist() == [0, 0, 0] and snap["refs"][0] == 3
    k0, _ = eng.pools[0]
    ids = snap["page_ids"][:, 1].tolist()
    assert len(set(ids)) == 3 and torch.equal(k0[ids[1]], k0[ids[0]]) and torch.equal(k0[ids[2]], k0[ids[0]]) and bool(k0[ids[0]].any())
    R.check_invariant(_state(eng))
    with np.errstate(all="ignore"):
        eng.step()                                                          # greedy: the branches stay one text
    assert eng.tokens.tolist() == [eng.tokens.tolist()[0]] * 3 and eng.lengths.tolist() == [73] * 3
    eng.pager.check(starved=True)


def test_a_follower_without_a_page_ends_with_no_pages(built_lib, monkeypatch):
    from qserve_amd import stopping
    D, rec, make = _engine(monkeypatch, page_pool=4)
    with np.errstate(all="ignore"):
        eng = _ready(make)
        eng.admit([0], [_tokens(70, 1)], max_new_tokens=8, copy_rows=[[1, 2, ]])
    # 4 pages: the leader's 2, row 1's tail copy, and the leader's next step ... row 2 is refused its copy
    snap = eng.pager.snapshot()
    assert snap["owned"].tolist() == [2, 2, 2] and snap["count"] == 0
    eng.release_rows([0, 1, 2])
    with np.errstate(all="ignore"):
        eng.admit([0], [_tokens(130, 1)], max_new_tokens=8, copy_rows=[[1, 2]])
    snap = eng.pager.snapshot()                                             # 3 + 1: row 2 holds nothing
    assert snap["owned"].tolist() == [3, 3, 0] and snap["starved"].tolist() == [0, 0, 1] and sorted(snap["refs"].tolist()) == [1, 1, 2, 2]
    assert eng.finished.tolist() == [0, 0, stopping.NO_PAGES]
    R.check_invariant(_state(eng))


def test_refusals_fire_before_any_call(built_lib, monkeypatch):
    D, rec, make = _engine(monkeypatch)
    with pytest.raises(AssertionError, match="share_pages=True shares pages of a page pool"):
        D.DecodeEngine(D.TINY, 3, 200, 30, device="cpu", seed=3, share_pages=True)
    with pytest.raises(AssertionError, match="runs on one GPU"):
        D.DecodeEngine(D.TINY, 3, 200, 30, device="cpu", seed=3, page_pool=4, share_pages=True, tp_rank=0, tp_world=2)
    with np.errstate(all="ignore"):
        eng = _ready(make)
        eng.admit([0], [_tokens(70, 1)], max_new_tokens=8)
        plain = D.DecodeEngine(D.TINY, 3, 200, 30, device="cpu", seed=3, page_pool=9)
        plain.enable_drafting(None)
        static = D.DecodeEngine(D.TINY, 3, 200, 30, device="cpu", seed=3)
        static.enable_drafting(None)
    assert plain.pager.refs is None and plain.prefix is None and eng.pager.refs is not None and eng.prefix is None
    at = len(rec.lines)
    for e in (plain, static):
        with pytest.raises(AssertionError, match="counted page pool"):
            e.fork(0, [1])
        with pytest.raises(AssertionError, match="counted page pool"):
            e.admit([0], [_tokens(70, 1)], copy_rows=[[1]])
    for rows in ([0], [1, 1], [3], []):
        with pytest.raises(AssertionError, match="distinct row indices"):
            eng.fork(0, rows)
    for rows, copies in (([0, 1], [[1], []]), ([0], [[0]]), ([0], [[1, 1]]), ([0], [[3]])):
        with pytest.raises(AssertionError, match="distinct row indices in 0 .. 2 overall"):
            eng.admit(rows, [_tokens(70, 1)] * len(rows), copy_rows=copies)
    with pytest.raises(AssertionError, match="one list of further rows per prompt"):
        eng.admit([0], [_tokens(70, 1)], copy_rows=[[1], [2]])
    assert len(rec.lines) == at and eng.pager.free_pages() == 7
