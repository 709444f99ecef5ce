"""The counted page pool kernels (qserve_amd/csrc/page_pool.hip: the reserve with `refs`, hold, unhold) against the numpy restatements
of tests/_page_ref_cases.py, through paging.PagePool(refcounts=True): bit-equal on every state tensor - `refs` and the order of the free
stack included - and on every table entry after every launch, the scratch zero again; every broken invariant sets `error` and changes
nothing; a counted pool that never shares is, op for op, the uncounted pool of tests/_page_cases.py."""
import numpy as np
import pytest
import torch

import _page_cases as P
import _page_ref_cases as R

pytestmark = pytest.mark.gpu

PB = 256


def _pool(gpu, B, mb, L, N):
    from qserve_amd import paging
    tables = [torch.zeros((B, 2, mb), dtype=torch.int64, device=gpu) for _ in range(L)]
    pools = [(torch.zeros((N + 1, PB), dtype=torch.uint8, device=gpu), torch.zeros((N + 1, PB), dtype=torch.uint8, device=gpu)) for _ in range(L)]
    pool = paging.PagePool(tables, pools, PB, refcounts=True)
    return pool, R.new_state(B, mb, L, N, PB, bases=pool.layer_bases.cpu().numpy())


def _seen(pool, st):
    return dict(pool.snapshot(), bases=st["bases"], N=st["N"], mb=st["mb"], page_bytes=PB)


def _dev(a, gpu):
    return None if a is None else torch.from_numpy(np.asarray(a, np.int32).copy()).to(gpu)


def _apply(pool, op, gpu):
    """One launch (through the wrapper where it takes the op as it is, through the entry where the op is one the wrapper refuses on the
    host) -> `finished` as the kernel left it (or None)."""
    from qserve_amd._lib import lib
    from qserve_amd.backend._util import check, ptr, stream
    if op["kind"] == "poke":
        t = getattr(pool, op["key"])
        if op["at"] is None:
            t.fill_(op["value"])
        else:
            t[op["at"]] = op["value"]
        return None
    if op["kind"] == "reserve":
        fin = _dev(op["finished"], gpu)
        pool.reserve(_dev(op["lengths"], gpu), op["extra"], extra_rows=_dev(op["extra_rows"], gpu), finished=fin)
        return None if fin is None else fin.cpu().numpy()
    ids = op["hold_ids"] if op["kind"] == "hold" else op["drop_ids"]
    ids_t = _dev(ids, gpu) if len(ids) else None
    tail = (len(ids), pool.B, pool.mb, pool.L, pool.N, pool.page_bytes, stream())
    if op["kind"] == "hold":                                               # (raw: take and src as the case words them)
        take, src = _dev(op["take"], gpu), _dev(op["src"], gpu)
        check(lib.qs_pages_hold(*pool._state(), ptr(pool.refs), ptr(pool._scratch), ptr(take), ptr(src), ptr(ids_t), *tail), "hold")
    else:
        mask = _dev(op["mask"], gpu)
        check(lib.qs_pages_unhold(*pool._state(), ptr(pool.refs), ptr(pool._scratch), ptr(mask), ptr(ids_t), *tail), "unhold")
    torch.cuda.synchronize()
    return None


def _run(gpu, B, mb, L, N, ops, what, broken=False):
    pool, st = _pool(gpu, B, mb, L, N)
    assert R.same_state(_seen(pool, st), st) is None
    cache, poked = set(), False
    for i, op in enumerate(ops):
        fin = _apply(pool, op, gpu)
        prev = st
        st, want_fin = R.apply_loop(prev, op)
        assert R.same_state(R.apply_arrays(prev, op)[0], st) is None
        got = _seen(pool, st)
        assert R.same_state(got, st) is None, f"{what}, op {i} ({op['kind']}): {R.same_state(got, st)} differs from the restatement"
        assert (fin is None and want_fin is None) or np.array_equal(fin, want_fin), f"{what}, op {i}: finished"
        assert not pool._scratch.any(), f"{what}, op {i}: the scratch is not zero again"
        poked = poked or op["kind"] == "poke"
        if broken and i == len(ops) - 1:
            assert got["error"] == 1
            with pytest.raises(RuntimeError, match="broken invariant"):
                pool.check()
        else:
            assert got["error"] == 0
            cache = R.cache_after(cache, op, False)
            if not poked:
                R.check_invariant(got, cache)
    return pool, st


@pytest.mark.parametrize("name", sorted(R.named_cases()))
def test_the_kernels_are_the_rule_on_every_named_case(gpu, name):
    _run(gpu, *R.named_cases()[name], what=name, broken=name in R.BROKEN)


@pytest.mark.parametrize("seed,shape", [(0, (5, 4, 7)), (1, (37, 5, 90)), (2, (9, 3, 12)), (3, (70, 6, 300))])
def test_random_sequences_keep_the_invariant(gpu, seed, shape):
    B, mb, N = shape
    _run(gpu, B, mb, 3, N, R.random_ops(np.random.default_rng(seed), B, mb, 3, N, 80), what=f"random {seed}")


def test_the_wrapper_takes_dicts_and_lists(gpu):
    """paging.PagePool.hold / release(drop_ids=) lower onto the entries: the named case `row_and_cache_together` through them."""
    pool, st = _pool(gpu, 5, 4, 2, 7)
    ops = R.named_cases()["row_and_cache_together"][4]
    pool.reserve(_dev(ops[0]["lengths"], gpu), 0, extra_rows=_dev(ops[0]["extra_rows"], gpu))
    pool.hold({}, hold_ids=[3, 1])
    pool.release(pool.rows_mask([1]))
    pool.hold({2: [0, 1], 4: [1]})
    pool.release(pool.rows_mask([2, 4]))
    pool.release(pool.rows_mask([0]), drop_ids=[3, 1])
    for op in ops:
        st, _ = R.apply_loop(st, op)
    got = _seen(pool, st)
    assert got["count"] == 7 and not got["refs"].any() and np.array_equal(got["free"], st["free"])
    R.check_invariant(got)
    pool.check()
    with pytest.raises(RuntimeError, match="page ids in 0"):
        pool.hold({1: [7]})


def test_a_counted_pool_that_never_shares_is_the_uncounted_pool(gpu):
    rng = np.random.default_rng(11)
    B, mb, N = 37, 5, 90
    pool, _ = _pool(gpu, B, mb, 3, N)
    st = P.new_state(B, mb, 3, N, PB, bases=pool.layer_bases.cpu().numpy())
    for i, op in enumerate(P.random_ops(rng, B, mb, 150)):
        if op["kind"] == "release":
            pool.release(_dev(op["mask"], gpu))
            fin = None
        else:
            fin = _dev(op["finished"], gpu)
            pool.reserve(_dev(op["lengths"], gpu), op["extra"], extra_rows=_dev(op["extra_rows"], gpu), finished=fin)
        st, want_fin = P.apply_loop(st, op)
        got = _seen(pool, st)
        assert P.same_state(got, st) is None, (i, op["kind"], P.same_state(got, st))
        assert fin is None or np.array_equal(fin.cpu().numpy(), want_fin)
        P.check_invariant(got)
        R.check_invariant(got)


def test_counted_launches_replay_from_a_captured_graph(gpu):
    """The counted reserve and an unhold in one graph over persistent argument tensors: two replays equal the restatement."""
    B, mb, L, N = 5, 4, 2, 7
    pool, st = _pool(gpu, B, mb, L, N)
    lengths, finished, mask = _dev(P.BOUNDARY, gpu), _dev([0] * B, gpu), _dev([0] * B, gpu)
    warm, _ = _pool(gpu, B, mb, L, N)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        warm.reserve(lengths, 1, finished=finished)
        warm.release(mask)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pool.reserve(lengths, 1, finished=finished)
        pool.release(mask)
    for lens, fin, rows in ((P.BOUNDARY, [0, 0, 0, 0, 0], [0, 1, 0, 0, 1]), ([129, 1, 64, 200, 70], [0, 0, 2, 0, 0], [1, 0, 0, 1, 0])):
        lengths.copy_(_dev(lens, gpu)), finished.copy_(_dev(fin, gpu)), mask.copy_(_dev(rows, gpu))
        g.replay()
        torch.cuda.synchronize()
        st, want_fin = R.reserve_loop(st, np.asarray(lens, np.int32), 1, None, np.asarray(fin, np.int32))
        st = R.unhold_loop(st, np.asarray(rows, np.int32), [])
        got = _seen(pool, st)
        assert R.same_state(got, st) is None, R.same_state(got, st)
        assert np.array_equal(finished.cpu().numpy(), want_fin)
        R.check_invariant(got)
