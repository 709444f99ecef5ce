"""GPU tests of the device-side tail of tree verification (qserve_amd.append: accept_greedy, commit_path_layers;
DecodeEngine.verify_tree(device_walk=True), capture_verify / run_verify): the walk against the plain-Python rule of
tests/_accept_cases.py, the all-layers commit against per-layer commit_path calls byte for byte, the device-walk engine against the
host path, and the captured verification against an eager twin (in a process of its own)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from _accept_cases import MALFORMED, random_cases, reference_walk
from _append_cases import scattered_tables
from _helpers import DevPools, dev

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KV = [pytest.param(True, id="kv4"), pytest.param(False, id="kv8")]


# ---- 1. the walk ----------------------------------------------------------------------------------------------------------------
class _Boxed:
    """A tensor of `shape` / `dtype` between two 4 KiB areas of 0xA5, itself filled with 0xA5."""

    def __init__(self, shape, dtype, device):
        nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        self.raw = torch.full((8192 + nbytes,), 0xA5, dtype=torch.uint8, device=device)
        self.t = self.raw[4096:4096 + nbytes].view(dtype).view(shape)

    def check(self, what):
        assert bool((self.raw[:4096] == 0xA5).all()) and bool((self.raw[-4096:] == 0xA5).all()), f"write outside {what}"


SENTINEL = int(np.array([0xA5] * 8, np.uint8).view(np.int64)[0])      # what an unwritten int64 entry of a box holds


def _check_accept(gpu, cases, cap):
    """One launch over the sequences `cases` (each (parents, tokens, argmax), possibly empty) against reference_walk."""
    from qserve_amd import append as A
    ns = [len(c[0]) for c in cases]
    batch, T = len(cases), sum(ns)
    cu = np.concatenate([[0], np.cumsum(ns)]).astype(np.int32)
    par = np.asarray([p for c in cases for p in c[0]], np.int64).astype(np.int32)
    tok = np.asarray([t for c in cases for t in c[1]], np.int64)
    am = np.asarray([a for c in cases for a in c[2]], np.int64)
    boxes = (_Boxed((batch, cap), torch.int32, gpu), _Boxed((batch,), torch.int32, gpu), _Boxed((batch,), torch.int64, gpu),
             _Boxed((batch,), torch.int64, gpu))
    out = A.accept_greedy(dev(tok), dev(am), dev(par), dev(cu), max_accept=cap, out=tuple(b.t for b in boxes))
    torch.cuda.synchronize()
    assert all(o is b.t for o, b in zip(out, boxes))
    for b, name in zip(boxes, ("accept_idx", "accept_lens", "last_row", "next_token")):
        b.check(name)
    idx, lens, last, nxt = (o.cpu().tolist() for o in out)
    for b, (p, t, a) in enumerate(cases):
        path = reference_walk(p, t, a, cap)
        assert lens[b] == len(path), f"sequence {b}: length {lens[b]}, expected {len(path)}"
        assert idx[b] == path + [0] * (cap - len(path)), f"sequence {b}: path {idx[b]}, expected {path} then zeros"
        if path:
            assert last[b] == int(cu[b]) + path[-1] and nxt[b] == a[path[-1]], f"sequence {b}: last_row / next_token"
        else:
            assert last[b] == -1 and nxt[b] == SENTINEL, f"sequence {b}: an empty sequence has last_row -1 and leaves next_token alone"
    return lens


def test_accept_on_the_random_cases_in_ragged_batches(gpu):
    """The 200 cases whose path-length mix tests/test_tree_accept_cpu.py pins, seven per launch plus an empty sequence that moves
    through the batch."""
    cases = random_cases()
    seen = []
    for i, s in enumerate(range(0, len(cases), 7)):
        batch = list(cases[s:s + 7])
        batch.insert(i % (len(batch) + 1), ([], [], []))
        seen += _check_accept(gpu, batch, 24)
    assert sum(x >= 3 for x in seen) >= 60 and sum(x == 1 for x in seen) >= 30 and seen.count(0) == 29


def test_accept_edge_shapes(gpu):
    one = ([-1], [7], [7])
    chain = ([-1] + list(range(63)), [99] + list(range(1, 64)), list(range(1, 64)) + [1234567890123])      # every node accepted
    assert _check_accept(gpu, [one], 1) == [1]
    assert _check_accept(gpu, [one, ([], [], []), one], 64) == [1, 0, 1]
    assert _check_accept(gpu, [chain, one], 64) == [64, 1]                    # the path fills all 64 entries
    assert _check_accept(gpu, [chain, one, chain], 5) == [5, 1, 5]            # max_accept below the path's length
    cases = random_cases()[:8]
    assert max(len(reference_walk(p, t, a, 24)) for p, t, a in cases) > 2
    _check_accept(gpu, cases, 2)
    # a wide tree: 63 children of the root, only the last one matches - the others differ from the arg-max beyond bit 32 only
    big = 1 << 40
    star = ([-1] + [0] * 63, [0] + [big << 1] * 62 + [big], [big] + [0] * 63)
    assert _check_accept(gpu, [star], 64) == [2]


def test_accept_on_malformed_parents(gpu):
    """Tokens and arg-max all 0: every edge the rule can follow is followed.  The walk ends, strictly increasing, inside the sequence."""
    cases = [(p, [0] * len(p), [0] * len(p)) for p in MALFORMED]
    lens = _check_accept(gpu, cases, 64)
    assert lens[0] == 1 and lens[3] == 3


def test_accept_allocates_its_outputs(gpu):
    from qserve_amd import append as A
    p, t, a = random_cases()[0]
    idx, lens, last, nxt = A.accept_greedy(dev(np.asarray(t, np.int64)), dev(np.asarray(a, np.int64)), dev(np.asarray(p, np.int32)),
                                           dev(np.asarray([0, 0, 24], np.int32)))
    torch.cuda.synchronize()
    path = reference_walk(p, t, a, 24)
    assert tuple(idx.shape) == (2, 24) and idx[1].tolist() == path + [0] * (24 - len(path)) and lens.tolist() == [0, len(path)]
    assert last.tolist() == [-1, path[-1]] and nxt.tolist() == [0, a[path[-1]]]


# ---- 2. the commit of every layer in one launch -----------------------------------------------------------------------------------
@pytest.mark.parametrize("int4", KV)
@pytest.mark.parametrize("Hkv", [1, 8])
def test_commit_path_layers_is_commit_path_per_layer(gpu, Hkv, int4):
    """L = 3 layers with tables and pools of their own, random page bytes, spare pages 0xFF.  Pasts 60 (the moves cross a page
    boundary), 64 (the shift: every source is the next move's destination) and 0 (a first page); the pools after ONE
    commit_path_layers against twin pools after three commit_path calls."""
    from qserve_amd import append as A
    L, n, mb = 3, 64, 3
    pasts = [60, 64, 0]
    lists = [[0, 2, 3, 5, 9, 30, 63], list(range(1, 64)), [0, 3, 4, 10]]      # (2 <- 3 while 1 <- 2: a source that is a destination)
    r = np.random.default_rng(7 * Hkv + int(int4))
    spt = Hkv * (64 if int4 else 128)
    idx = np.zeros((len(pasts), n), np.int32)
    for b, path in enumerate(lists):
        idx[b, : len(path)] = path
    past, idx_d, lens_d = dev(np.asarray(pasts, np.int32)), dev(idx), dev(np.asarray([len(x) for x in lists], np.int32))
    pools, twins, tables, kvps, twin_kvps = [], [], [], [], []
    for li in range(L):
        t, nblocks = scattered_tables(r, len(pasts), mb)
        p, q = DevPools(nblocks, Hkv, int4, gpu), DevPools(nblocks, Hkv, int4, gpu)
        for which, pool in ((0, p.k), (1, p.v)):
            used = sorted(set(t[:, which].ravel().tolist()))
            pool[used] = dev(r.integers(0, 256, size=(len(used), p.pb), dtype=np.uint8))
        q.k.copy_(p.k)
        q.v.copy_(p.v)
        pools.append(p), twins.append(q), tables.append(t), kvps.append(p.pointers(t)), twin_kvps.append(q.pointers(t))
    start = [(p.k.clone(), p.v.clone()) for p in pools]
    lt = A.layer_table_pointers(kvps)
    assert lt.dtype == torch.int64 and lt.tolist() == [k.data_ptr() for k in kvps]
    A.commit_path_layers(lt, past, idx_d, lens_d, mb, Hkv, spt, int4)
    for kvp in twin_kvps:
        A.commit_path(kvp, past, idx_d, lens_d, Hkv, spt, int4)
    torch.cuda.synchronize()
    for li in range(L):
        assert torch.equal(pools[li].k, twins[li].k) and torch.equal(pools[li].v, twins[li].v), f"layer {li}: pages differ from commit_path's"
        assert not torch.equal(pools[li].k, start[li][0]) and not torch.equal(pools[li].v, start[li][1]), f"layer {li}: nothing moved"
        for which, pool in ((0, pools[li].k), (1, pools[li].v)):
            spare = [i for i in range(pool.size(0)) if i not in set(tables[li][:, which].ravel().tolist())]
            assert spare and bool((pool[spare] == 0xFF).all()), f"layer {li}: a page of no sequence was written"
    with pytest.raises(RuntimeError, match="tables are"):
        A.commit_path_layers(lt, past, idx_d, lens_d, mb + 1, Hkv, spt, int4)      # a max_blocks the tables do not have


# ---- 3. the engine: device walk against the host path ---------------------------------------------------------------------------
def test_engine_device_walk_is_the_host_path(gpu):
    """Two engines on the same prompt, the tree and drafts of tests/test_append_tree_gpu.py::test_engine_verify_tree: one verifies on
    the host path, one with device_walk=True.  Results and state agree bit for bit - after the first call, after a second one on the
    now ragged lengths, and after a step() on each."""
    import _accept_engine as E
    toks = E.prompt(gpu)
    rng = np.random.default_rng(3)
    draft = E.greedy_draft(E.engine(toks), rng, gpu)
    host, walk = E.engine(toks), E.engine(toks)
    E.assert_same_state(host, walk, "after prefill")
    a = host.verify_tree(draft, E.PAR)
    b = walk.verify_tree(draft, E.PAR, device_walk=True)
    E.assert_same_result(a, b, "first verify")
    E.assert_same_state(host, walk, "first verify")
    assert torch.equal(host.final.view(torch.int16), walk.final.view(torch.int16))
    lens1 = a[1].tolist()
    print(f"engine: accepted path lengths {lens1}")
    assert max(lens1) >= 2, "the greedy continuation was accepted nowhere: only root-only paths were compared"
    draft2 = E.random_draft(rng, gpu)
    a2 = host.verify_tree(draft2, E.PAR)
    b2 = walk.verify_tree(draft2, E.PAR, device_walk=True)
    E.assert_same_result(a2, b2, "second verify")
    E.assert_same_state(host, walk, "second verify")
    host.step()
    walk.step()
    E.assert_same_state(host, walk, "step() after the verifications")
    # the host-side bound of the lengths: an upper bound throughout, exact again on request
    assert walk._len_bound >= int(walk.lengths.max()) and host._len_bound >= int(host.lengths.max())
    assert walk.sync_length_bound() == int(walk.lengths.max())
    # the per-tree constants are built once
    assert list(walk._tree_cache) == [tuple(E.PAR)]


# ---- 4. capture -------------------------------------------------------------------------------------------------------------------
def test_capture_verify_replays_against_an_eager_twin(gpu):
    """tests/_accept_engine.py as a program, in a fresh process: capture_verify, two run_verify calls with different drafts, an eager
    device-walk twin.  A capture that succeeds is also the proof that no host synchronisation is left in the path."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_accept_engine.py")], cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and "CAPTURE-OK" in r.stdout, f"exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
