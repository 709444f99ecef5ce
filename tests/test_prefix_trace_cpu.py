"""DecodeEngine(prefix_cache=True).admit on the host (the recorder and stubs of tests/test_engine_trace_cpu.py, the stand-ins of the
counted page entries of tests/test_page_refs_contracts.py): a prompt without a hit launches unhold, the counted reserve, the whole
prompt's passes and - behind the one read-back - the cache's holds; a prompt with a hit launches unhold, hold, the counted reserve and
passes over the uncached tokens alone at past c_r + c0; the refusals fire before any call."""
import numpy as np
import pytest
import torch

import _page_ref_cases as R


def _engine(monkeypatch, batch=3, **kw):
    import qserve_amd.backend._util as U
    import test_engine_trace_cpu as T
    import test_page_refs_contracts as C
    from qserve_amd import paging
    from qserve_amd._lib import SIGNATURES, lib
    D, rec = T.install(monkeypatch)
    for attr in ("stream", "expect", "guard"):
        monkeypatch.setattr(paging, attr, getattr(U, attr))
    for name, fn in C.FAKES.items():
        monkeypatch.setattr(lib, name, rec.wrap(name, fn, SIGNATURES[name][1]))
    kw = dict(dict(page_pool=9, prefix_cache=True), **kw)
    return D, rec, (lambda: rec.watch(D.DecodeEngine(D.TINY, batch, 200, 30, device="cpu", seed=3, **kw)))


def _tokens(n, seed):
    return torch.randint(0, 512, (n,), generator=torch.Generator().manual_seed(seed))


def _passes(D, monkeypatch):
    """Record (past_lens, tokens per sequence) of every `append.append` call at the Python seam."""
    from qserve_amd import append as A
    real, seen = A.append, []

    def append(qkv, cu_seqlens_q, past_lens, *args, **kw):
        seen.append((past_lens.tolist(), np.diff(cu_seqlens_q.numpy()).tolist(), kw.get("max_past")))
        return real(qkv, cu_seqlens_q, past_lens, *args, **kw)

    monkeypatch.setattr(A, "append", append)
    return seen


def _state(eng):
    p = eng.pager
    return dict(p.snapshot(), bases=p.layer_bases.numpy(), N=p.N, mb=p.mb, page_bytes=p.page_bytes)


def test_admit_maps_what_is_cached_and_runs_the_rest(built_lib, monkeypatch):
    D, rec, make = _engine(monkeypatch)
    eng = make()
    L = len(eng.layers)
    eng.enable_drafting(None, max_ngram=3, min_match=1, pad_token=7)
    eng.set_stopping((), 0)
    seen = _passes(D, monkeypatch)
    X = _tokens(150, 1)
    Y, Z = torch.cat((X[:128], _tokens(61, 2))), torch.cat((X[:64], _tokens(30, 3)))
    page = lambda at: [line.split()[0] for line in rec.lines[at:] if line.startswith("pages_")]      # noqa: E731
    with np.errstate(all="ignore"):
        at = len(rec.lines)
        eng.admit([0], [X], max_new_tokens=8, chunk=128)
        # nothing cached: no hold in front, the whole prompt in passes [0, 128) and [128, 150), then the cache's holds of two pages
        assert page(at) == ["pages_unhold", "pages_reserve_refs", "pages_hold"] and rec.lines[at].startswith("pages_unhold")
        assert seen == [([0], [128], 0)] * L + [([128], [22], 128)] * L
        assert eng.pager.refs.tolist()[:3] == [2, 2, 1] and eng._row_cached == {0: [0, 1]} and len(eng.prefix) == 2
        del seen[:]
        at = len(rec.lines)
        eng.admit([2, 1], [Z, Y], max_new_tokens=8, chunk=128)
    # hits of one and two pages: unhold, hold, the counted reserve - then passes over the uncached tokens alone, at past c_r + c0;
    # Z computes 30 tokens behind 64, Y 61 behind 128; nothing new for the cache (Z's 94 tokens fill no second page): no further hold
    assert page(at) == ["pages_unhold", "pages_hold", "pages_reserve_refs"]
    assert [line.split()[0] for line in rec.lines[at:at + 3]] == page(at)
    assert seen == [([64, 128], [30, 61], 128)] * L
    snap = eng.pager.snapshot()
    assert snap["owned"].tolist() == [3, 3, 2] and snap["page_ids"][1, :2].tolist() == [0, 1] and snap["page_ids"][2, 0] == 0
    assert snap["refs"].tolist()[:2] == [4, 3] and snap["count"] == 9 - 5 and snap["error"] == 0
    assert eng._row_cached == {0: [0, 1], 1: [0, 1], 2: [0]} and eng.lengths.tolist() == [151, 190, 95]
    R.check_invariant(_state(eng), cache=[0, 1])
    # a second admit into row 2 gives its holds up first, and the text is again what was asked for
    with np.errstate(all="ignore"):
        eng.admit([2], [_tokens(70, 9)], max_new_tokens=8)
    assert eng._row_cached[2] == [4] and eng.pager.refs.tolist()[:2] == [3, 3] and len(eng.prefix) == 3
    R.check_invariant(_state(eng), cache=[0, 1, 4])
    # releasing rows tells the cache; eviction is one unhold launch with the ids
    eng.release_rows([0, 1, 2])
    assert eng.prefix.evictable() == 3 and eng.pager.free_pages() == 6
    at = len(rec.lines)
    assert sorted(eng.evict_prefixes(9)) == [0, 1, 4] and page(at) == ["pages_unhold"]
    assert eng.pager.free_pages() == 9 and not eng.pager.refs.any() and eng.evict_prefixes(1) == [] and page(at) == ["pages_unhold"]


def test_refusals_fire_before_any_call(built_lib, monkeypatch):
    D, rec, make = _engine(monkeypatch)
    with pytest.raises(AssertionError, match="give page_pool=N"):
        D.DecodeEngine(D.TINY, 3, 200, 30, device="cpu", seed=3, prefix_cache=True)
    with pytest.raises(AssertionError, match="page_pool=4 - a page pool"):
        D.DecodeEngine(D.TINY, 3, 200, 30, device="cpu", seed=3, page_pool=4, prefix_cache=True, tp_rank=0, tp_world=2)
    eng = make()
    eng.enable_lora(2, 8)
    eng.enable_drafting(None)
    eng.set_lora([0, -1, 1])
    at = len(rec.lines)
    with pytest.raises(AssertionError, match=r"set_lora\(None\) before admitting"):
        eng.admit([0], [_tokens(70, 1)])
    with pytest.raises(AssertionError, match="no reference counts"):
        eng.prefill_shared(_tokens(64, 1), _tokens(3 * 4, 2).view(3, 4))
    assert len(rec.lines) == at and len(eng.prefix) == 0 and eng.pager.free_pages() == 9
    plain = D.DecodeEngine(D.TINY, 3, 200, 30, device="cpu", seed=3, page_pool=4)
    with pytest.raises(AssertionError, match="no prefix cache"):
        plain.evict_prefixes(1)
    assert plain.prefix is None and plain.pager.refs is None
