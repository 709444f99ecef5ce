"""Contracts of the counted page pool that need no GPU: the header declares the three entries, their argument validation (before any
HIP call), and the lowering of paging.PagePool(refcounts=True) onto them - through host-memory stand-ins of the entries written here
over the loop restatement of tests/_page_ref_cases.py (tests/test_prefix_trace_cpu.py runs the engine over the same stand-ins)."""
import os
import re

import numpy as np
import pytest
import torch

import _page_ref_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_header_declares_the_three_entries():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qserve_amd.h")).read(), flags=re.S)
    for name in ("qs_pages_reserve_refs", "qs_pages_hold", "qs_pages_unhold"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", txt), name
    from qserve_amd import _lib
    assert [len(_lib.SIGNATURES[n][1]) for n in ("qs_pages_reserve_refs", "qs_pages_hold", "qs_pages_unhold")] == [19, 20, 19]
    # the two uncounted entries stay as they were
    assert len(_lib.SIGNATURES["qs_pages_reserve"][1]) == 18 and len(_lib.SIGNATURES["qs_pages_release"][1]) == 15


def test_argument_validation_without_gpu(built_lib):
    from qserve_amd._lib import lib
    state = dict(free=4096, count=8192, ids=12288, owned=16384, starved=20480, error=24576, tables=28672, bases=32768, refs=45056)

    def head(s):
        return [s[k] for k in ("free", "count", "ids", "owned", "starved", "error", "tables", "bases", "refs")]

    def reserve(lengths=36864, extra_rows=None, finished=None, batch=2, mb=4, L=2, N=7, pb=256, extra=1, **change):
        return lib.qs_pages_reserve_refs(*head({**state, **change}), lengths, extra_rows, finished, batch, mb, L, N, pb, extra, None)

    def hold(take=36864, src=40960, more=None, n=0, scratch=49152, batch=2, mb=4, L=2, N=7, pb=256, **change):
        return lib.qs_pages_hold(*head({**state, **change}), scratch, take, src, more, n, batch, mb, L, N, pb, None)

    def unhold(mask=36864, more=None, n=0, scratch=49152, batch=2, mb=4, L=2, N=7, pb=256, **change):
        return lib.qs_pages_unhold(*head({**state, **change}), scratch, mask, more, n, batch, mb, L, N, pb, None)

    for call, rows in ((reserve, ("lengths",)), (hold, ("take", "src", "scratch")), (unhold, ("mask", "scratch"))):
        for bad in (*state, *rows):
            assert call(**{bad: None}) == -1 and b"null pointer" in lib.qs_last_error(), (call.__name__, bad)
        for name in ("free", "count", "ids", "owned", "starved", "error", "refs", *rows):
            assert call(**{name: 4098}) == -1 and b"4-byte" in lib.qs_last_error(), (call.__name__, name)
        for name in ("tables", "bases"):
            assert call(**{name: 28676}) == -1 and b"8-byte" in lib.qs_last_error(), name
        assert call(N=0) == -1 and b"num_pages=0" in lib.qs_last_error()
        assert call(mb=0) == -1 and call(L=0) == -1 and b"num_layers=0" in lib.qs_last_error()
        assert call(pb=0) == -1 and b"page_bytes=0" in lib.qs_last_error()
        assert call(N=1 << 29) == -1 and b"2^30" in lib.qs_last_error()
        assert call(batch=-1) == -1 and call(batch=1025) == -1 and b"batch=1025" in lib.qs_last_error()
        assert call(batch=1024, mb=1 << 19) == -1 and b"2^31" in lib.qs_last_error()
        assert call(batch=0) == 0                                           # nothing to do: no launch
    assert reserve(extra=-1) == -1 and b"extra=-1" in lib.qs_last_error()
    for name in ("extra_rows", "finished"):
        assert reserve(**{name: 40962}) == -1 and b"4-byte" in lib.qs_last_error(), name
    for call in (hold, unhold):
        assert call(n=-1) == -1 and b"-1 ids" in lib.qs_last_error()
        assert call(more=53248, n=8) == -1 and b"8 ids" in lib.qs_last_error()      # more ids than pages
        assert call(more=None, n=1) == -1 and b"null id list" in lib.qs_last_error()
        assert call(more=53250, n=1) == -1 and b"4-byte" in lib.qs_last_error()
        assert call(more=53248, n=0, batch=0) == 0


# ---- the three entries over host memory ------------------------------------------------------------------------------------------------
def _views(state_args, refs, batch, mb, L, N, pb):
    import _fake_abi as F
    import test_page_pool_contracts as C
    views, tabs, st = C._state_views(*state_args, batch, mb, L, N, pb)
    views["refs"] = F._arr(refs, (N,), np.int32)
    st["refs"] = views["refs"].copy()
    return views, tabs, st


def _write_back(views, tabs, out):
    import test_page_pool_contracts as C
    C._write_back(views, tabs, out)
    views["refs"][:] = out["refs"]


def _fake_reserve_refs(free, count, page_ids, owned, starved, error, layer_tables, layer_bases, refs, lengths, extra_rows, finished, batch,
                       mb, L, N, pb, extra, stream):
    import _fake_abi as F
    F.CALLS.append(("qs_pages_reserve_refs", batch, mb, L, N, pb, extra, bool(extra_rows), bool(finished)))
    views, tabs, st = _views((free, count, page_ids, owned, starved, error, layer_tables, layer_bases), refs, batch, mb, L, N, pb)
    fin = F._arr(finished, (batch,), np.int32) if finished else None
    out, new_fin = R.reserve_loop(st, F._arr(lengths, (batch,), np.int32), extra, F._arr(extra_rows, (batch,), np.int32) if extra_rows else None, fin)
    _write_back(views, tabs, out)
    if fin is not None:
        fin[:] = new_fin
    return 0


def _fake_hold(free, count, page_ids, owned, starved, error, layer_tables, layer_bases, refs, scratch, take, src, hold_ids, num_hold, batch,
               mb, L, N, pb, stream):
    import _fake_abi as F
    F.CALLS.append(("qs_pages_hold", batch, mb, L, N, pb, num_hold))
    views, tabs, st = _views((free, count, page_ids, owned, starved, error, layer_tables, layer_bases), refs, batch, mb, L, N, pb)
    ids = F._arr(hold_ids, (num_hold,), np.int32) if num_hold else np.zeros((0,), np.int32)
    _write_back(views, tabs, R.hold_loop(st, F._arr(take, (batch,), np.int32), F._arr(src, (batch, mb), np.int32), ids))
    return 0


def _fake_unhold(free, count, page_ids, owned, starved, error, layer_tables, layer_bases, refs, scratch, rows_mask, drop_ids, num_drop, batch,
                 mb, L, N, pb, stream):
    import _fake_abi as F
    F.CALLS.append(("qs_pages_unhold", batch, mb, L, N, pb, num_drop))
    views, tabs, st = _views((free, count, page_ids, owned, starved, error, layer_tables, layer_bases), refs, batch, mb, L, N, pb)
    ids = F._arr(drop_ids, (num_drop,), np.int32) if num_drop else np.zeros((0,), np.int32)
    _write_back(views, tabs, R.unhold_loop(st, F._arr(rows_mask, (batch,), np.int32), ids))
    return 0


FAKES = dict(qs_pages_reserve_refs=_fake_reserve_refs, qs_pages_hold=_fake_hold, qs_pages_unhold=_fake_unhold)


def _host_pool(monkeypatch, refcounts=True, B=5, mb=4, L=2, N=7, pb=256):
    import _fake_abi as F
    import qserve_amd.backend._util as U
    from qserve_amd import append, paging
    from qserve_amd._lib import lib
    calls = F.install(monkeypatch)
    for name, fn in FAKES.items():
        monkeypatch.setattr(lib, name, fn, raising=True)
    for m in (paging, append):
        for attr in ("stream", "expect", "guard"):
            monkeypatch.setattr(m, attr, getattr(U, attr))
    tables = [torch.zeros((B, 2, mb), dtype=torch.int64) for _ in range(L)]
    pools = [(torch.zeros((N + 1, pb), dtype=torch.uint8), torch.zeros((N + 1, pb), dtype=torch.uint8)) for _ in range(L)]
    return paging.PagePool(tables, pools, pb, refcounts=refcounts), calls


def _restated(pool):
    return dict(pool.snapshot(), bases=pool.layer_bases.numpy(), N=pool.N, mb=pool.mb, page_bytes=pool.page_bytes)


def test_the_counted_wrapper_lowers_onto_the_three_entries(built_lib, monkeypatch):
    pool, calls = _host_pool(monkeypatch)
    st = R.new_state(5, 4, 2, 7, 256, bases=pool.layer_bases.numpy())
    assert R.same_state(_restated(pool), st) is None
    ops = R.named_cases()["row_and_cache_together"][4]
    pool.reserve(torch.from_numpy(ops[0]["lengths"]), 0, extra_rows=torch.from_numpy(ops[0]["extra_rows"]))
    assert calls[-1] == ("qs_pages_reserve_refs", 5, 4, 2, 7, 256, 0, True, False)
    pool.hold({}, hold_ids=[3, 1])
    assert calls[-1] == ("qs_pages_hold", 5, 4, 2, 7, 256, 2)
    pool.release(pool.rows_mask([1]))
    assert calls[-1] == ("qs_pages_unhold", 5, 4, 2, 7, 256, 0)
    pool.release(torch.tensor([True, False, False, False, False]), drop_ids=[3, 1])
    assert calls[-1] == ("qs_pages_unhold", 5, 4, 2, 7, 256, 2)
    for op in ops:
        st, _ = R.apply_loop(st, op)
    assert R.same_state(_restated(pool), st) is None and pool.free_pages() == 7
    pool.reserve(torch.ones(5, dtype=torch.int32), 0, extra_rows=torch.tensor([100, 0, 0, 0, 0], dtype=torch.int32))
    ids = pool.snapshot()["page_ids"][0, :2].tolist()
    pool.hold({3: ids, 4: ids[:1]})
    snap = pool.snapshot()
    assert snap["owned"].tolist() == [2, 0, 0, 2, 1] and snap["refs"][ids].tolist() == [3, 2]
    R.check_invariant(_restated(pool))
    pool.check()
    # what the wrapper refuses on the host, and what check() says of a broken invariant
    for match, call in (("rows are 0", lambda: pool.hold({5: [0]})), ("page ids in 0", lambda: pool.hold({1: [7]})),
                        ("at most 4 page ids", lambda: pool.hold({1: [0] * 5})), ("hold_ids", lambda: pool.hold({}, hold_ids=[-1])),
                        ("drop_ids", lambda: pool.release(pool.rows_mask([]), drop_ids=[9]))):
        with pytest.raises(RuntimeError, match=match):
            call()
    pool.hold({0: ids})                                                     # into a row that owns pages
    with pytest.raises(RuntimeError, match="into a row that owns"):
        pool.check()


def test_an_uncounted_pool_has_no_holds(built_lib, monkeypatch):
    pool, calls = _host_pool(monkeypatch, refcounts=False)
    assert pool.refs is None and "refs" not in pool.snapshot()
    with pytest.raises(RuntimeError, match="refcounts=True"):
        pool.hold({0: [1]})
    with pytest.raises(RuntimeError, match="refcounts=True"):
        pool.release(pool.rows_mask([0]), drop_ids=[1])
    assert not calls
