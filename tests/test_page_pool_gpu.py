"""The page pool kernels (qserve_amd/csrc/page_pool.hip) against the numpy restatements of tests/_page_cases.py: bit-equal on every
state tensor and on every table entry of every layer (`base + id * page_bytes`, or the sink) after every launch - the named cases (the
boundary lengths at extra = 1 and 12, starvation, a finished mask, release and reuse, extra_rows, batches that cross a wave and the
workgroup's stride), 200 random ops, one reserve and one release replayed from a captured graph, and a corrupted count, free entry, `owned` and `page_ids` entry."""
import numpy as np
import pytest
import torch

import _page_cases as P

pytestmark = pytest.mark.gpu

PB = 256                                                                    # bytes of a page here: the kernels never touch a page


def _pool(gpu, B, mb, L, N):
    from qserve_amd import paging
    tables = [torch.zeros((B, 2, mb), dtype=torch.int64, device=gpu) for _ in range(L)]
    pools = [(torch.zeros((N + 1, PB), dtype=torch.uint8, device=gpu), torch.zeros((N + 1, PB), dtype=torch.uint8, device=gpu)) for _ in range(L)]
    pool = paging.PagePool(tables, pools, PB)
    return pool, P.new_state(B, mb, L, N, PB, bases=pool.layer_bases.cpu().numpy())


def _seen(pool, st):
    return dict(pool.snapshot(), bases=st["bases"], N=st["N"], mb=st["mb"], page_bytes=PB)


def _dev(a, gpu):
    return None if a is None else torch.from_numpy(np.asarray(a, np.int32).copy()).to(gpu)


def _apply(pool, op, gpu):
    """One launch -> `finished` as the kernel left it (or None)."""
    if op["kind"] == "release":
        pool.release(_dev(op["mask"], gpu))
        return None
    fin = _dev(op["finished"], gpu)
    pool.reserve(_dev(op["lengths"], gpu), op["extra"], extra_rows=_dev(op["extra_rows"], gpu), finished=fin)
    return None if fin is None else fin.cpu().numpy()


def _run(gpu, B, mb, L, N, ops, what):
    pool, st = _pool(gpu, B, mb, L, N)
    assert P.same_state(_seen(pool, st), st) is None
    for i, op in enumerate(ops):
        fin = _apply(pool, op, gpu)
        prev = st
        st, want_fin = P.apply_loop(prev, op)
        assert P.same_state(P.apply_arrays(prev, op)[0], st) is None       # (the two restatements agree on this very op)
        got = _seen(pool, st)
        assert P.same_state(got, st) is None, f"{what}, op {i} ({op['kind']}): {P.same_state(got, st)} differs from the restatement"
        assert (fin is None and want_fin is None) or np.array_equal(fin, want_fin), f"{what}, op {i}: finished"
        P.check_invariant(got)
    return pool, st


@pytest.mark.parametrize("name", sorted(P.named_cases()))
def test_the_kernels_are_the_rule_on_every_named_case(gpu, name):
    _run(gpu, *P.named_cases()[name], what=name)


def test_two_hundred_random_ops_keep_the_invariant(gpu):
    rng = np.random.default_rng(11)
    B, mb, N = 37, 5, 90
    _run(gpu, B, mb, 3, N, P.random_ops(rng, B, mb, 200), what="random")


def test_eager_equals_captured_replay(gpu):
    """One reserve and one release captured in one graph over persistent argument tensors: two replays, each on refilled arguments,
    leave what the restatement leaves."""
    B, mb, L, N = 5, 4, 2, 7
    pool, st = _pool(gpu, B, mb, L, N)
    lengths, finished, mask = _dev(P.BOUNDARY, gpu), _dev([0] * B, gpu), _dev([0] * B, gpu)
    warm, _ = _pool(gpu, B, mb, L, N)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                              # (a warm-up outside the capture, on a pool of its own)
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
        st, want_fin = P.reserve_loop(st, np.asarray(lens, np.int32), 1, None, np.asarray(fin, np.int32))
        st = P.release_loop(st, np.asarray(rows, np.int32))
        got = _seen(pool, st)
        assert P.same_state(got, st) is None, P.same_state(got, st)
        assert np.array_equal(finished.cpu().numpy(), want_fin)
        P.check_invariant(got)


@pytest.mark.parametrize("count", [8, -1])
def test_a_corrupted_count_sets_error_and_changes_nothing(gpu, count):
    ops = P.named_cases()["step"][4]
    pool, st = _run(gpu, 5, 4, 2, 7, ops, what="step")
    pool.count.fill_(count)
    before = pool.snapshot()
    fin = _dev([0] * 5, gpu)
    pool.reserve(_dev([200] * 5, gpu), 12, finished=fin)
    pool.release(_dev([1] * 5, gpu))
    after = pool.snapshot()
    assert after["error"] == 1 and before["error"] == 0 and not fin.any()
    for k in ("free", "count", "page_ids", "owned", "starved", "tables"):
        assert np.array_equal(after[k], before[k]), k
    with pytest.raises(RuntimeError, match="broken invariant"):
        pool.check()


@pytest.mark.parametrize("what", ["free", "owned_high", "owned_negative", "page_ids"])
def test_a_corrupted_entry_sets_error_and_changes_nothing(gpu, what):
    """The other invariants of the header, one launch each: a page id outside 0 .. N - 1 among those about to be popped, an `owned`
    outside 0 .. mb (both entries), a page id outside 0 .. N - 1 among those about to be pushed.  (Every index is clamped before an
    address is formed from it: the launches touch nothing beyond the state.)"""
    pool, st = _run(gpu, 5, 4, 2, 7, P.named_cases()["step"][4][:1], what="step")
    snap = pool.snapshot()
    assert snap["count"] >= 1 and snap["owned"][1] >= 2
    grow0 = lambda: pool.reserve(_dev([64 * int(snap["owned"][0]) + 1, 1, 1, 1, 1], gpu), 1)      # noqa: E731  (row 0 pops one page)
    release = lambda: pool.release(_dev([1] * 5, gpu))                                              # noqa: E731
    if what == "free":
        pool.free[snap["count"] - 1] = 7                                    # the page row 0 would pop: the sink's index
        launches = [grow0]
    elif what == "page_ids":
        pool.page_ids[1, 1] = -3
        launches = [release]
    else:
        pool.owned[2] = 5 if what == "owned_high" else -1
        launches = [grow0, release]
    for launch in launches:
        pool.error.zero_()
        before = pool.snapshot()
        launch()
        after = pool.snapshot()
        assert after["error"] == 1 and before["error"] == 0
        for k in ("free", "count", "page_ids", "owned", "starved", "tables"):
            assert np.array_equal(after[k], before[k]), k
    with pytest.raises(RuntimeError, match="broken invariant"):
        pool.check()
