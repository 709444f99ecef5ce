"""Contracts of the page pool that need no GPU: the header declares both entries, their argument validation (which happens before any
HIP call), the argument checks of qserve_amd.paging and its lowering onto the C ABI - through a host-memory stand-in of the two entries
written here, over the loop restatement of tests/_page_cases.py -, and the engine's call sequence: a pooled engine launches one reserve
at the head of step, verify and speculate, an engine without a pool launches none."""
import os
import re

import numpy as np
import pytest
import torch

import _page_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_header_declares_both_entries():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qserve_amd.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+qs_pages_reserve\s*\(", txt) and re.search(r"\bint\s+qs_pages_release\s*\(", txt)
    from qserve_amd import _lib
    assert len(_lib.SIGNATURES["qs_pages_reserve"][1]) == 18 and len(_lib.SIGNATURES["qs_pages_release"][1]) == 15
    from qserve_amd import stopping
    assert stopping.NO_PAGES == 3 == P.NO_PAGES


def test_argument_validation_without_gpu(built_lib):
    from qserve_amd._lib import lib
    state = dict(free=4096, count=8192, ids=12288, owned=16384, starved=20480, error=24576, tables=28672, bases=32768)

    def reserve(lengths=36864, extra_rows=None, finished=None, batch=2, mb=4, L=2, N=7, pb=256, extra=1, **change):
        s = {**state, **change}
        return lib.qs_pages_reserve(s["free"], s["count"], s["ids"], s["owned"], s["starved"], s["error"], s["tables"], s["bases"], lengths,
                                    extra_rows, finished, batch, mb, L, N, pb, extra, None)

    def release(mask=36864, batch=2, mb=4, L=2, N=7, pb=256, **change):
        s = {**state, **change}
        return lib.qs_pages_release(s["free"], s["count"], s["ids"], s["owned"], s["starved"], s["error"], s["tables"], s["bases"], mask,
                                    batch, mb, L, N, pb, None)

    for call, rows in ((reserve, "lengths"), (release, "mask")):
        for bad in (*state, rows):
            assert call(**{bad: None}) == -1 and b"null pointer" in lib.qs_last_error(), bad
        for name in ("free", "count", "ids", "owned", "starved", "error", rows):
            assert call(**{name: 4098}) == -1 and b"4-byte" in lib.qs_last_error(), name
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
        assert reserve(**{name: 40960}, batch=0) == 0
    assert reserve(batch=0, extra=0, N=1, mb=1, L=1, pb=1) == 0


# ---- the two entries over host memory ----------------------------------------------------------------------------------------------
def _state_views(free, count, page_ids, owned, starved, error, layer_tables, layer_bases, batch, mb, L, N, pb):
    import _fake_abi as F
    tabs = [F._arr(int(a), (batch, 2, mb), np.int64) for a in F._arr(layer_tables, (L,), np.int64)]
    views = dict(free=F._arr(free, (N,), np.int32), count=F._arr(count, (1,), np.int32), page_ids=F._arr(page_ids, (batch, mb), np.int32),
                 owned=F._arr(owned, (batch,), np.int32), starved=F._arr(starved, (batch,), np.int32), error=F._arr(error, (1,), np.int32))
    st = dict({k: v.copy() for k, v in views.items()}, tables=np.stack(tabs), bases=F._arr(layer_bases, (L, 2), np.int64).copy(), N=N, mb=mb,
              page_bytes=pb)
    st["count"], st["error"] = int(st["count"][0]), int(st["error"][0])
    return views, tabs, st


def _write_back(views, tabs, out):
    for k in ("free", "page_ids", "owned", "starved"):
        views[k][:] = out[k]
    views["count"][0], views["error"][0] = out["count"], out["error"] or views["error"][0]
    for t, new in zip(tabs, out["tables"]):
        t[:] = new


def _fake_reserve(free, count, page_ids, owned, starved, error, layer_tables, layer_bases, lengths, extra_rows, finished, batch, mb, L, N, pb,
                  extra, stream):
    import _fake_abi as F
    F.CALLS.append(("qs_pages_reserve", batch, mb, L, N, pb, extra, bool(extra_rows), bool(finished)))
    views, tabs, st = _state_views(free, count, page_ids, owned, starved, error, layer_tables, layer_bases, batch, mb, L, N, pb)
    fin = F._arr(finished, (batch,), np.int32) if finished else None
    out, new_fin = P.reserve_loop(st, F._arr(lengths, (batch,), np.int32), extra, F._arr(extra_rows, (batch,), np.int32) if extra_rows else None, fin)
    _write_back(views, tabs, out)
    if fin is not None:
        fin[:] = new_fin
    return 0


def _fake_release(free, count, page_ids, owned, starved, error, layer_tables, layer_bases, rows_mask, batch, mb, L, N, pb, stream):
    import _fake_abi as F
    F.CALLS.append(("qs_pages_release", batch, mb, L, N, pb))
    views, tabs, st = _state_views(free, count, page_ids, owned, starved, error, layer_tables, layer_bases, batch, mb, L, N, pb)
    _write_back(views, tabs, P.release_loop(st, F._arr(rows_mask, (batch,), np.int32)))
    return 0


def _host_pool(monkeypatch, B=5, mb=4, L=2, N=7, pb=256):
    """A paging.PagePool over host tensors and the stand-ins -> (the pool, the calls)."""
    import _fake_abi as F
    import qserve_amd.backend._util as U
    from qserve_amd import append, paging
    from qserve_amd._lib import lib
    calls = F.install(monkeypatch)
    monkeypatch.setattr(lib, "qs_pages_reserve", _fake_reserve, raising=True)
    monkeypatch.setattr(lib, "qs_pages_release", _fake_release, raising=True)
    for m in (paging, append):
        for attr in ("stream", "expect", "guard"):
            monkeypatch.setattr(m, attr, getattr(U, attr))
    tables = [torch.zeros((B, 2, mb), dtype=torch.int64) for _ in range(L)]
    pools = [(torch.zeros((N + 1, pb), dtype=torch.uint8), torch.zeros((N + 1, pb), dtype=torch.uint8)) for _ in range(L)]
    return paging.PagePool(tables, pools, pb), calls


def _restated(pool):
    """The restatement's view of a host pool: its snapshot plus the constants."""
    return dict(pool.snapshot(), bases=pool.layer_bases.numpy(), N=pool.N, mb=pool.mb, page_bytes=pool.page_bytes)


def test_the_wrapper_lowers_onto_the_abi(built_lib, monkeypatch):
    """qserve_amd.paging over the stand-ins: a new pool is the restatement's new state (all free, page 0 on top, every entry the sink);
    batch / max_blocks / layers / pages / page_bytes come from the shapes; `extra`, the optional arrays and a bool mask arrive as the
    header orders them; snapshot, free_pages and check read what the launches left."""
    pool, calls = _host_pool(monkeypatch)
    st = P.new_state(5, 4, 2, 7, 256, bases=pool.layer_bases.numpy())
    assert P.same_state(_restated(pool), st) is None
    P.check_invariant(_restated(pool))
    t = lambda a: None if a is None else torch.from_numpy(np.asarray(a, np.int32).copy())   # noqa: E731
    for name in ("step", "finished_mask", "release_reuse", "extra_rows"):
        for op in P.named_cases()[name][4]:
            if op["kind"] == "reserve":
                fin = t(op["finished"])
                pool.reserve(t(op["lengths"]), op["extra"], extra_rows=t(op["extra_rows"]), finished=fin)
                assert calls[-1] == ("qs_pages_reserve", 5, 4, 2, 7, 256, op["extra"], op["extra_rows"] is not None, fin is not None)
                st, want_fin = P.reserve_arrays(st, op["lengths"], op["extra"], op["extra_rows"], op["finished"])
                assert fin is None or np.array_equal(fin.numpy(), want_fin)
            else:
                pool.release(t(op["mask"]).bool() if name == "release_reuse" else t(op["mask"]))
                assert calls[-1] == ("qs_pages_release", 5, 4, 2, 7, 256)
                st = P.release_arrays(st, op["mask"])
            assert P.same_state(_restated(pool), st) is None, (name, P.same_state(_restated(pool), st))
            P.check_invariant(_restated(pool))
            assert pool.free_pages() == st["count"]
        pool.release(pool.rows_mask(range(5)))
        st = P.release_arrays(st, np.ones((5,), np.int32))
    pool.check()
    pool.reserve(t([250, 256, 1, 1, 1]), 1)                                  # row 1 starves, and every growing row behind it
    pool.check()
    with pytest.raises(RuntimeError, match=r"rows \[1, 2, 3, 4\] were refused pages"):
        pool.check(starved=True)
    pool.count.fill_(9)
    pool.release(pool.rows_mask([0]))
    with pytest.raises(RuntimeError, match="broken invariant"):
        pool.check()


def test_paging_argument_checks(built_lib, monkeypatch):
    """Wrong dtypes, shapes and values are reported with the argument's name before anything is launched."""
    from qserve_amd import paging
    pool, calls = _host_pool(monkeypatch)
    n = len(calls)
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32)             # noqa: E731

    def bad(match, fn, *args, **kw):
        with pytest.raises(RuntimeError, match=match):
            fn(*args, **kw)

    bad("lengths", pool.reserve, i32(5).long(), 1)
    bad("lengths must be", pool.reserve, i32(4), 1)
    bad("extra_rows must be", pool.reserve, i32(5), 1, extra_rows=i32(5, 1))
    bad("finished", pool.reserve, i32(5), 1, finished=i32(5).long())
    bad("extra=-1", pool.reserve, i32(5), -1)
    bad("rows_mask must be", pool.release, i32(6))
    bad("rows_mask", pool.release, i32(5).long())
    bad("row indices", pool.rows_mask, [5])
    assert len(calls) == n
    tables = [torch.zeros((5, 2, 4), dtype=torch.int64) for _ in range(2)]
    pair = lambda rows=8, pb=256: (torch.zeros((rows, pb), dtype=torch.uint8), torch.zeros((rows, pb), dtype=torch.uint8))   # noqa: E731
    bad("one .K, V. pool pair per layer", paging.PagePool, tables, [pair()], 256)
    bad(r"pools\[1\]\[0\] must be", paging.PagePool, tables, [pair(), pair(9)], 256)
    bad(r"pools\[0\]\[0\] must be", paging.PagePool, tables, [pair(pb=128), pair(pb=128)], 256)
    bad("N >= 1", paging.PagePool, tables, [pair(1), pair(1)], 256)
    bad("page_bytes=0", paging.PagePool, tables, [pair(), pair()], 0)
    bad("every table must be", paging.PagePool, [torch.zeros((5, 3, 4), dtype=torch.int64)], [pair()], 256)
    pool.release(torch.ones((5,), dtype=torch.bool))                        # a bool mask is converted
    assert calls[-1][0] == "qs_pages_release"


# ---- the engine's call sequence ----------------------------------------------------------------------------------------------------
def _engine_lines(monkeypatch, page_pool):
    """The entries a TINY engine calls, per phase, on the host (the recorder and stubs of tests/test_engine_trace_cpu.py; the two page
    entries run the stand-ins above)."""
    import qserve_amd.backend._util as U
    import test_engine_trace_cpu as T
    from qserve_amd import paging
    from qserve_amd._lib import SIGNATURES, lib
    D, rec = T.install(monkeypatch)
    for attr in ("stream", "expect", "guard"):
        monkeypatch.setattr(paging, attr, getattr(U, attr))
    monkeypatch.setattr(lib, "qs_pages_reserve", rec.wrap("qs_pages_reserve", _fake_reserve, SIGNATURES["qs_pages_reserve"][1]))
    monkeypatch.setattr(lib, "qs_pages_release", rec.wrap("qs_pages_release", _fake_release, SIGNATURES["qs_pages_release"][1]))
    eng = rec.watch(D.DecodeEngine(D.TINY, 2, 5, 40, device="cpu", seed=3, page_pool=page_pool))
    toks = torch.randint(0, 512, (2 * 5,), generator=torch.Generator().manual_seed(1))
    phases = {}

    def phase(name, fn):
        at = len(rec.lines)
        with np.errstate(all="ignore"):
            fn()
        phases[name] = [line.split()[0] for line in rec.lines[at:]], rec.lines[at:]

    phase("prefill", lambda: eng.prefill(5, toks))
    phase("prefill_chunked", lambda: eng.prefill_chunked(5, 3, toks))
    eng.enable_drafting(toks, max_ngram=3, min_match=1, pad_token=7)
    phase("step", eng.step)
    phase("verify_host", lambda: eng.verify_tree(torch.zeros((2, len(T.PAR)), dtype=torch.int64), T.PAR))
    phase("verify_device", lambda: eng.verify_tree(torch.zeros((2, len(T.PAR)), dtype=torch.int64), T.PAR, device_walk=True))
    phase("speculate", lambda: eng.speculate(T.PAR))
    eng.set_stopping(stop=[3], max_new_tokens=30)
    phase("step_stopping", eng.step)
    phase("speculate_stopping", lambda: eng.speculate(T.PAR))
    return eng, phases


def test_a_pooled_engine_reserves_once_at_the_head_of_every_round(built_lib, monkeypatch):
    import test_engine_trace_cpu as T
    eng, phases = _engine_lines(monkeypatch, 7)                            # (7 pages: not the tree's 6 nodes)
    for name in ("step", "verify_host", "verify_device", "speculate", "step_stopping", "speculate_stopping"):
        names, lines = phases[name]
        assert names[0] == "pages_reserve" and names.count("pages_reserve") == 1 and "pages_release" not in names, (name, names[:3])
        words = lines[0].split()
        # ... lengths, extra_rows, finished, batch, max_blocks, layers, pages, page_bytes, extra, stream
        assert words[9] == "lengths" and words[10] == "0" and words[11] == ("finished" if name.endswith("stopping") else "0"), lines[0]
        assert words[12:16] == ["2", str(eng.mb), "2", "7"] and int(words[16]) == eng.page_bytes
        assert words[17] == ("1" if name.startswith("step") else str(len(T.PAR))), lines[0]
    for name in ("prefill", "prefill_chunked"):
        names, lines = phases[name]
        assert names[:2] == ["pages_release", "pages_reserve"] and names.count("pages_reserve") == 1 and names.count("pages_release") == 1
        assert lines[1].split()[9] == "_all_rows" and lines[1].split()[17] == "5"
    snap = eng.pager.snapshot()
    P.check_invariant(dict(snap, bases=eng.pager.layer_bases.numpy(), N=7, mb=eng.mb, page_bytes=eng.page_bytes))
    assert snap["owned"].tolist() == [1, 1] and snap["count"] == 5
    eng.set_stopping(None)
    with pytest.raises(AssertionError, match="page pool"):
        eng.prefill_shared(torch.zeros((70,), dtype=torch.int64), torch.zeros((2, 4), dtype=torch.int64))
    with pytest.raises(AssertionError, match="one GPU"):
        type(eng)(eng.cfg, 2, 5, 4, device="cpu", tp_rank=0, tp_world=2, page_pool=6)


def test_an_engine_without_a_pool_launches_neither_entry(built_lib, monkeypatch):
    eng, phases = _engine_lines(monkeypatch, None)
    assert eng.pager is None
    for name, (names, _) in phases.items():
        assert "pages_reserve" not in names and "pages_release" not in names, name
