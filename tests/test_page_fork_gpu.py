"""The fork kernels (qserve_amd/csrc/page_pool.hip: qs_pages_fork's two launches) against the numpy restatements of
tests/_page_fork_cases.py, through paging.PagePool(refcounts=True): bit-equal on every state tensor, every table entry and EVERY POOL
BYTE after every launch - the pools start as random bytes, so a missing or misplaced copy shows -; every broken invariant sets `error`
and changes nothing, no pool byte either.  Page sizes: 256 bytes (at most one vector per thread), 34 816 (the KV4 page of Llama-3-8B:
the strided vector loop) and 100 (no multiple of 16: the byte loop)."""
import numpy as np
import pytest
import torch

import _page_fork_cases as K

pytestmark = pytest.mark.gpu

SIZES = (256, 34816, 100)


def _pool(gpu, B, mb, L, N, pb, seed=0):
    from qserve_amd import paging
    g = torch.Generator().manual_seed(seed)
    tables = [torch.zeros((B, 2, mb), dtype=torch.int64, device=gpu) for _ in range(L)]
    pools = [tuple(torch.randint(0, 256, (N + 1, pb), generator=g, dtype=torch.uint8).to(gpu) for _ in range(2)) for _ in range(L)]
    pool = paging.PagePool(tables, pools, pb, refcounts=True)
    return pool, K.new_state(B, mb, L, N, pb, bases=pool.layer_bases.cpu().numpy(), pool_bytes=_bytes(pool))


def _bytes(pool):
    return torch.stack([torch.stack(pair) for pair in pool.pools]).cpu().numpy()


def _seen(pool, st):
    return dict(pool.snapshot(), bases=st["bases"], N=st["N"], mb=st["mb"], page_bytes=st["page_bytes"], bytes=_bytes(pool))


def _dev(a, gpu):
    return None if a is None else torch.from_numpy(np.asarray(a, np.int32).copy()).to(gpu)


def _apply(pool, op, gpu):
    """One op through the pool (fork: the tensor form of PagePool.fork takes src_rows as the case words them) -> `finished` as the
    kernel left it (or None)."""
    import test_page_refs_gpu as G
    if op["kind"] != "fork":
        return G._apply(pool, op, gpu)
    fin = _dev(op["finished"], gpu)
    pool.fork(_dev(op["src_rows"], gpu), _dev(op["lengths"], gpu), finished=fin)
    return None if fin is None else fin.cpu().numpy()


def _run(gpu, B, mb, L, N, ops, what, pb=256, broken=False):
    pool, st = _pool(gpu, B, mb, L, N, pb)
    assert K.same_state(_seen(pool, st), st) is None
    cache, poked = set(), False
    for i, op in enumerate(ops):
        fin = _apply(pool, op, gpu)
        prev = st
        st, want_fin = K.apply_loop(prev, op)
        if op["kind"] == "fork":
            assert K.same_state(K.apply_arrays(prev, op)[0], st) is None
        got = _seen(pool, st)
        assert K.same_state(got, st) is None, f"{what}, op {i} ({op['kind']}): {K.same_state(got, st)} differs from the restatement"
        assert (fin is None and want_fin is None) or np.array_equal(fin, want_fin), f"{what}, op {i}: finished"
        assert not pool._scratch.any()
        poked = poked or op["kind"] == "poke"
        if broken and i == len(ops) - 1:
            assert got["error"] == 1 and np.array_equal(got["bytes"], prev["bytes"])
            with pytest.raises(RuntimeError, match="broken invariant"):
                pool.check()
        else:
            assert got["error"] == 0
            cache = K.cache_after(cache, op, False)
            if not poked:
                K.check_invariant(got, cache)
    return pool, st


def _cases():
    """Every named case at 256-byte pages; those of a handful of pages at the real page and at the byte path too."""
    for name, (B, mb, L, N, ops) in sorted(K.named_cases().items()):
        for pb in SIZES if N < 16 else (256, 100) if name == "wave" else (256,):
            yield pytest.param(name, pb, id=f"{name}-{pb}")


@pytest.mark.parametrize("name,pb", list(_cases()))
def test_the_kernels_are_the_rule_on_every_named_case(gpu, name, pb):
    _run(gpu, *K.named_cases()[name], what=name, pb=pb, broken=name in K.BROKEN)


@pytest.mark.parametrize("seed,shape,pb", [(0, (5, 4, 7), 34816), (1, (37, 5, 90), 256), (2, (9, 3, 12), 100), (3, (70, 6, 300), 256)])
def test_random_sequences_keep_the_invariant(gpu, seed, shape, pb):
    B, mb, N = shape
    _run(gpu, B, mb, 3, N, K.random_ops(np.random.default_rng(seed), B, mb, 3, N, 80), what=f"random {seed}", pb=pb)


def test_the_wrapper_takes_a_dict(gpu):
    B, mb, L, N, ops = K.named_cases()["two_sources"]
    pool, st = _pool(gpu, B, mb, L, N, 256)
    pool.reserve(_dev(ops[0]["lengths"], gpu), 0, extra_rows=_dev(ops[0]["extra_rows"], gpu))
    pool.fork({1: 0, 2: 3, 4: 3}, _dev(ops[1]["lengths"], gpu))
    for op in ops:
        st, _ = K.apply_loop(st, op)
    assert K.same_state(_seen(pool, st), st) is None
    pool.check(starved=True)


def test_reserve_and_fork_replay_from_a_captured_graph(gpu):
    """The counted reserve and a fork in one graph over persistent argument tensors; two replays with different src_rows (and a release
    between them) equal the restatement, pool bytes included."""
    B, mb, L, N = 5, 4, 2, 9
    pool, st = _pool(gpu, B, mb, L, N, 34816)
    extra, lengths, src, finished = _dev([0] * B, gpu), _dev([1] * B, gpu), _dev([-1] * B, gpu), _dev([0] * B, gpu)
    ones = _dev([1] * B, gpu)
    warm, _ = _pool(gpu, B, mb, L, N, 34816)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        warm.reserve(ones, 0, extra_rows=extra)
        warm.fork(src, lengths, finished=finished)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pool.reserve(ones, 0, extra_rows=extra)
        pool.fork(src, lengths, finished=finished)
    rounds = (([70, 0, 0, 140, 0], [70, 1, 1, 140, 1], [-1, 0, 3, -1, 3], [0, 0, 0, 0, 2]),
              ([0, 0, 129, 0, 0], [1, 1, 129, 1, 1], [2, 2, -1, 2, 2], [0, 1, 0, 0, 0]))
    for k, (texts, lens, rows, fin) in enumerate(rounds):
        extra.copy_(_dev(texts, gpu)), lengths.copy_(_dev(lens, gpu)), src.copy_(_dev(rows, gpu)), finished.copy_(_dev(fin, gpu))
        g.replay()
        torch.cuda.synchronize()
        st, _ = K.R.reserve_loop(st, np.ones(B, np.int32), 0, np.asarray(texts, np.int32), None)
        st, want_fin = K.fork_loop(st, np.asarray(rows, np.int32), np.asarray(lens, np.int32), np.asarray(fin, np.int32))
        got = _seen(pool, st)
        assert K.same_state(got, st) is None, (k, K.same_state(got, st))
        assert np.array_equal(finished.cpu().numpy(), want_fin)
        K.check_invariant(got)
        if k == 0:
            assert got["owned"].tolist() == [2, 2, 3, 3, 3] and got["count"] == 1
            pool.release(pool.rows_mask(range(B)))
            st = K.R.unhold_loop(st, np.ones(B, np.int32), [])
    assert got["owned"].tolist() == [2, 2, 3, 2, 2] and got["refs"][got["page_ids"][2, :2]].tolist() == [5, 5]
