"""Contracts of the fork entry that need no GPU: the header declares it, its argument validation (before any HIP call), and the
lowering of paging.PagePool.fork onto it - through a host-memory stand-in written here over the loop restatement of
tests/_page_fork_cases.py, which copies the pools' bytes as the second launch does."""
import copy
import os
import re

import numpy as np
import pytest
import torch

import _page_fork_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_header_declares_the_entry_with_18_arguments():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qserve_amd.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+qs_pages_fork\s*\(([^;]*)\)\s*;", txt)
    assert m and len(m.group(1).split(",")) == 18
    from qserve_amd import _lib
    assert len(_lib.SIGNATURES["qs_pages_fork"][1]) == 18
    names = [a.split()[-1].lstrip("*") for a in m.group(1).split(",")]
    assert names[8:12] == ["refs", "src_rows", "lengths", "finished"] and names[12:] == ["batch", "max_blocks", "num_layers", "num_pages",
                                                                                        "page_bytes", "stream"]


def test_argument_validation_without_gpu(built_lib):
    from qserve_amd._lib import lib
    state = dict(free=4096, count=8192, ids=12288, owned=16384, starved=20480, error=24576, tables=28672, bases=32768, refs=45056)

    def fork(src_rows=36864, lengths=40960, finished=None, batch=2, mb=4, L=2, N=7, pb=256, **change):
        s = {**state, **change}
        return lib.qs_pages_fork(*[s[k] for k in ("free", "count", "ids", "owned", "starved", "error", "tables", "bases", "refs")], src_rows,
                                 lengths, finished, batch, mb, L, N, pb, None)

    for bad in (*state, "src_rows", "lengths"):
        assert fork(**{bad: None}) == -1 and b"null pointer" in lib.qs_last_error(), bad
    for name in ("free", "count", "ids", "owned", "starved", "error", "refs", "src_rows", "lengths", "finished"):
        assert fork(**{name: 4098}) == -1 and b"4-byte" in lib.qs_last_error(), name
    for name in ("tables", "bases"):
        assert fork(**{name: 28676}) == -1 and b"8-byte" in lib.qs_last_error(), name
    assert fork(N=0) == -1 and b"num_pages=0" in lib.qs_last_error()
    assert fork(mb=0) == -1 and fork(L=0) == -1 and b"num_layers=0" in lib.qs_last_error()
    assert fork(pb=0) == -1 and b"page_bytes=0" in lib.qs_last_error()
    assert fork(N=1 << 29) == -1 and b"2^30" in lib.qs_last_error()
    assert fork(batch=-1) == -1 and fork(batch=1025) == -1 and b"batch=1025" in lib.qs_last_error()
    assert fork(batch=1024, mb=1 << 19) == -1 and b"2^31" in lib.qs_last_error()
    assert fork(batch=0) == 0 and fork(batch=0, finished=49152) == 0          # nothing to do: no launch


# ---- the entry over host memory --------------------------------------------------------------------------------------------------------
def _fake_fork(free, count, page_ids, owned, starved, error, layer_tables, layer_bases, refs, src_rows, lengths, finished, batch, mb, L, N,
               pb, stream):
    import _fake_abi as F
    import test_page_refs_contracts as C
    F.CALLS.append(("qs_pages_fork", batch, mb, L, N, pb, bool(finished)))
    views, tabs, st = C._views((free, count, page_ids, owned, starved, error, layer_tables, layer_bases), refs, batch, mb, L, N, pb)
    pools = [[F._arr(int(a), (N + 1, pb), np.uint8) for a in pair] for pair in st["bases"]]
    st["bytes"] = np.array(pools)
    fin = F._arr(finished, (batch,), np.int32) if finished else None
    out, new_fin = K.fork_loop(st, F._arr(src_rows, (batch,), np.int32), F._arr(lengths, (batch,), np.int32), fin)
    C._write_back(views, tabs, out)
    for pair, new in zip(pools, out["bytes"]):
        pair[0][:], pair[1][:] = new[0], new[1]
    if fin is not None:
        fin[:] = new_fin
    return 0


def _host_pool(monkeypatch, refcounts=True, **shape):
    import test_page_refs_contracts as C
    from qserve_amd._lib import lib
    pool, calls = C._host_pool(monkeypatch, refcounts=refcounts, **shape)
    monkeypatch.setattr(lib, "qs_pages_fork", _fake_fork, raising=True)
    g = torch.Generator().manual_seed(5)
    for pair in pool.pools:
        for t in pair:
            t.copy_(torch.randint(0, 256, t.shape, generator=g, dtype=torch.uint8))
    return pool, calls


def _restated(pool):
    """The restatement's view of a host pool, copied: the snapshot of a host pool is its memory."""
    return copy.deepcopy(dict(pool.snapshot(), bases=pool.layer_bases.numpy(), N=pool.N, mb=pool.mb, page_bytes=pool.page_bytes,
                              bytes=np.array([[k.numpy(), v.numpy()] for k, v in pool.pools])))


def test_fork_lowers_onto_the_entry(built_lib, monkeypatch):
    pool, calls = _host_pool(monkeypatch)
    t = lambda a: torch.from_numpy(np.asarray(a, np.int32).copy())         # noqa: E731
    ops = K.named_cases()["two_sources"]
    pool2, _ = _host_pool(monkeypatch, N=9)
    st = _restated(pool2)
    reserve, fork = ops[4]
    pool2.reserve(t(reserve["lengths"]), 0, extra_rows=t(reserve["extra_rows"]))
    pool2.fork({1: 0, 2: 3, 4: 3}, t(fork["lengths"]))                      # a dict, uploaded once ...
    assert calls[-1] == ("qs_pages_fork", 5, 4, 2, 9, 256, False)
    for op in ops[4]:
        st, _ = K.apply_loop(st, op)
    assert K.same_state(_restated(pool2), st) is None
    K.check_invariant(_restated(pool2))
    # ... or the tensor the entry takes, with `finished`
    ops = K.named_cases()["free_ends_midway_finished"][4]
    pool3, _ = _host_pool(monkeypatch, B=7)
    st = _restated(pool3)
    pool3.reserve(t(ops[0]["lengths"]), 0, extra_rows=t(ops[0]["extra_rows"]))
    fin = t(ops[1]["finished"])
    n = len(calls)
    pool3.fork(t(ops[1]["src_rows"]), t(ops[1]["lengths"]), finished=fin)
    assert calls[n:] == [("qs_pages_fork", 7, 4, 2, 7, 256, True)]          # one call of the entry
    for op in ops:
        st, want_fin = K.apply_loop(st, op)
    assert K.same_state(_restated(pool3), st) is None and np.array_equal(fin.numpy(), want_fin)
    pool3.check()
    with pytest.raises(RuntimeError, match=r"rows \[4, 5\] were refused pages"):
        pool3.check(starved=True)
    # what the wrapper refuses on the host, and what check() says of a broken invariant
    n = len(calls)
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32)             # noqa: E731
    for match, call in (("rows are 0", lambda: pool.fork({5: 0}, i32(5))), ("rows are 0", lambda: pool.fork({1: -1}, i32(5))),
                        ("its own source", lambda: pool.fork({1: 1}, i32(5))), ("src_rows must be", lambda: pool.fork(i32(4), i32(5))),
                        ("src_rows", lambda: pool.fork(i32(5).long(), i32(5))), ("lengths must be", lambda: pool.fork({1: 0}, i32(6))),
                        ("finished", lambda: pool.fork({1: 0}, i32(5), finished=i32(5).long()))):
        with pytest.raises(RuntimeError, match=match):
            call()
    assert len(calls) == n
    pool.fork({2: 0, 3: 2}, torch.ones(5, dtype=torch.int32))               # off a destination of the same launch
    with pytest.raises(RuntimeError, match="off a destination of the same launch"):
        pool.check()


def test_an_uncounted_pool_cannot_fork(built_lib, monkeypatch):
    pool, calls = _host_pool(monkeypatch, refcounts=False)
    with pytest.raises(RuntimeError, match="refcounts=True"):
        pool.fork({1: 0}, torch.ones(5, dtype=torch.int32))
    assert not calls
