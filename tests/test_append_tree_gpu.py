"""GPU parity of tree-draft verification (qserve_amd.append: append_tree_rope_update_kv_cache, append_tree_attention, commit_path;
DecodeEngine.verify_tree): chains against the linear entries bit for bit, random trees and arbitrary words against the float64 oracle
of tests/_tree_cases.py, leaks, the path commit byte for byte, and the engine."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from _append_cases import host_pool, scattered_tables
from _helpers import DevPools, dev
from _tree_cases import as_int64, chain_words, depths, expected_tree, random_parents, rotate_rows_tree, words_from_parents
from oracle import kvattn

pytestmark = pytest.mark.gpu
TOL = 2e-3      # the TOL of tests/test_append_gpu.py: an fp16 MFMA attention against a float64 oracle on standard normal inputs
BASE = 1e4
KV = [pytest.param(True, id="kv4"), pytest.param(False, id="kv8")]


def _spt(Hkv, int4):
    return Hkv * (64 if int4 else 128)


def _np(t):
    return t.detach().cpu().numpy()


def _prefill_write(qkv, lens, kvp, H, Hkv, int4):
    """The existing prefill writer over whole sequences (in place on qkv and the pages)."""
    from qserve_backend import fused_attention as fa
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    mx = int(max(lens))
    pad = fa.compute_padding_offsets(dev(cu), mx, int(cu[-1]))
    fa.apply_bias_rope_update_kv_cache(qkv, dev(np.asarray(lens, np.int32)), pad, kvp, H, Hkv, mx, 64, _spt(Hkv, int4), 128, BASE,
                                       8192, True, int4, True)


class _Canaried:
    """out [T, H, 128] fp16 between two 4 KiB areas of 0xA5."""

    def __init__(self, T, H, device):
        self.raw = torch.full((8192 + T * H * 256,), 0xA5, dtype=torch.uint8, device=device)
        self.out = self.raw[4096:4096 + T * H * 256].view(torch.float16).view(T, H, 128)

    def check(self):
        assert bool((self.raw[:4096] == 0xA5).all()) and bool((self.raw[-4096:] == 0xA5).all()), "write outside `out`"


def _spare_blocks_untouched(pools, tables, nblocks):
    used_k, used_v = set(tables[:, 0].ravel().tolist()), set(tables[:, 1].ravel().tolist())
    for name, pool, used in (("K", pools.k, used_k), ("V", pools.v, used_v)):
        spare = [i for i in range(nblocks) if i not in used]
        assert spare and bool((pool[spare] == 0xFF).all()), f"a {name} page of no sequence was written"


class _Case:
    """A cache holding `pasts` tokens per sequence (existing prefill writer, 0xFF-filled pools, scattered tables) and `ns` new rows."""

    def __init__(self, gpu, H, Hkv, int4, pasts, ns, seed, extra_blocks=1):
        self.r = r = np.random.default_rng(seed)
        self.H, self.Hkv, self.int4, self.gpu = H, Hkv, int4, gpu
        self.B, self.W = len(pasts), (H + 2 * Hkv) * 128
        mb = (max(p + n for p, n in zip(pasts, ns)) + 63) // 64 + extra_blocks
        self.tables, self.nblocks = scattered_tables(r, self.B, mb)
        self.pools = DevPools(self.nblocks, Hkv, int4, gpu)
        self.kvp = self.pools.pointers(self.tables)
        live = [b for b in range(self.B) if pasts[b] > 0]
        if live:
            ctx = dev(r.standard_normal((sum(pasts[b] for b in live), self.W)).astype(np.float16))
            _prefill_write(ctx, [pasts[b] for b in live], self.pools.pointers(self.tables[live]), H, Hkv, int4)
        self.T = int(sum(ns))
        self.new = r.standard_normal((self.T, self.W)).astype(np.float16)
        self.cu_q = np.concatenate([[0], np.cumsum(ns)]).astype(np.int32)
        self.past = np.asarray(pasts, np.int32)
        self.ns = list(ns)
        self.spt = _spt(Hkv, int4)

    def clone_pools(self):
        p = DevPools(self.nblocks, self.Hkv, self.int4, self.gpu)
        p.k.copy_(self.pools.k)
        p.v.copy_(self.pools.v)
        return p

    def host(self, pools=None):
        pools = pools or self.pools
        return host_pool(_np(pools.k), _np(pools.v), self.Hkv, self.int4)


# ---- 1. a chain is the linear entries, bit for bit ------------------------------------------------------------------------------
@pytest.mark.parametrize("int4", KV)
@pytest.mark.parametrize("H,Hkv", [(8, 2), (4, 4), (7, 1)])
def test_chain_masks_give_the_linear_entries_bit_for_bit(gpu, H, Hkv, int4):
    """Same tiles, same values masked, same order: torch.equal on the rotated rows, the pages and the outputs (un-split and with
    the same forced split count)."""
    from qserve_amd import append as A
    c = _Case(gpu, H, Hkv, int4, [0, 1, 63, 64, 130], [64, 5, 0, 33, 1], seed=3 * H + Hkv + int(int4))
    cu_q, past = dev(c.cu_q), dev(c.past)
    masks = A.tree_masks_from_parents([p for n in c.ns for p in range(-1, n - 1)], c.cu_q).to(gpu)
    assert [int(x) & (2 ** 64 - 1) for x in masks.tolist()] == [w for n in c.ns for w in chain_words(n)]
    lin_pools = c.clone_pools()
    a, b = dev(c.new), dev(c.new)
    A.append_rope_update_kv_cache(a, cu_q, past, lin_pools.pointers(c.tables), H, Hkv, c.spt, BASE, int4)
    A.append_tree_rope_update_kv_cache(b, cu_q, past, c.kvp, masks, H, Hkv, c.spt, BASE, int4)
    torch.cuda.synchronize()
    assert torch.equal(a, b), "rotated qkv rows differ"
    assert torch.equal(lin_pools.k, c.pools.k) and torch.equal(lin_pools.v, c.pools.v), "pages differ"
    _spare_blocks_untouched(c.pools, c.tables, c.nblocks)
    for splits in (None, 3):
        box = _Canaried(c.T, H, gpu)
        lin = A.append_attention(a, cu_q, past, c.kvp, H, Hkv, c.spt, int4, max_seqlen_q=64, num_splits=splits)
        tree = A.append_tree_attention(b, cu_q, past, c.kvp, masks, H, Hkv, c.spt, int4, max_seqlen_q=64, num_splits=splits, out=box.out)
        torch.cuda.synchronize()
        box.check()
        assert torch.isfinite(tree).all() and torch.equal(lin, tree), f"num_splits={splits}: tree attention differs from the linear entry"


# ---- 2. random closed trees against float64 -------------------------------------------------------------------------------------
@pytest.mark.parametrize("int4", KV)
@pytest.mark.parametrize("H,Hkv", [(32, 8), (6, 2), (5, 1), (16, 8)])
def test_random_trees_against_the_float64_oracle(gpu, H, Hkv, int4):
    from qserve_amd import append as A
    c = _Case(gpu, H, Hkv, int4, [0, 37, 200, 64], [64, 17, 40, 1], seed=11 * H + Hkv + int(int4))
    parents = [p for n in c.ns for p in random_parents(c.r, n)]
    words = [w for s, e in zip(c.cu_q, c.cu_q[1:]) for w in words_from_parents(parents[s:e])]
    masks = A.tree_masks_from_parents(parents, c.cu_q)
    assert np.array_equal(masks.numpy(), as_int64(words))
    assert max(depths(words[:64], 64)) < 63, "the first tree is a chain: nothing tested"
    masks = masks.to(gpu)
    cu_q, past = dev(c.cu_q), dev(c.past)
    qkv = dev(c.new)
    before = c.host()
    A.append_tree_rope_update_kv_cache(qkv, cu_q, past, c.kvp, masks, H, Hkv, c.spt, BASE, int4)
    torch.cuda.synchronize()
    rot = _np(qkv)
    # q and k of node i sit at position past + depth(i), bit for bit oracle.kvattn.rope_neox; v is untouched
    assert np.array_equal(rot.view(np.uint16), rotate_rows_tree(c.new, c.cu_q, c.past, words, H, Hkv, BASE).view(np.uint16))
    ref = expected_tree(rot, c.cu_q, c.past, c.tables, before, H, Hkv, words)      # (only positions < past are read)
    for splits in (1, 2, 7):
        box = _Canaried(c.T, H, gpu)
        out = A.append_tree_attention(qkv, cu_q, past, c.kvp, masks, H, Hkv, c.spt, int4, max_seqlen_q=64, num_splits=splits, out=box.out)
        torch.cuda.synchronize()
        box.check()
        got = _np(out).astype(np.float64)
        assert np.isfinite(got).all()
        err = np.abs(got - ref).max()
        print(f"tree attention H={H} Hkv={Hkv} int4={int4} splits={splits}: max abs err {err:.3e}")
        assert err <= TOL, f"num_splits={splits}: max abs err {err:.2e}"
    _spare_blocks_untouched(c.pools, c.tables, c.nblocks)


# ---- 2b. no workspace yet: the un-split tree launch ------------------------------------------------------------------------------
_CHILD = r"""
import sys
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import numpy as np, torch
from _append_cases import host_pool, scattered_tables
from _helpers import DevPools, dev
from _tree_cases import expected_tree, words_from_parents
from qserve_amd import append as A
from qserve_backend import fused_attention as fa
gpu = torch.device("cuda:0")
H, Hkv, int4, B, past_len, n, BASE = 8, 2, True, 2, 200, 3, 1e4
spt = Hkv * 64
r = np.random.default_rng(6)
W = (H + 2 * Hkv) * 128
tables, nblocks = scattered_tables(r, B, 5)
pools = DevPools(nblocks, Hkv, int4, gpu)
kvp = pools.pointers(tables)
ctx = dev(r.standard_normal((B * past_len, W)).astype(np.float16))
cu = dev(np.array([0, past_len, 2 * past_len], np.int32))
fa.apply_bias_rope_update_kv_cache(ctx, dev(np.array([past_len] * B, np.int32)), fa.compute_padding_offsets(cu, past_len, B * past_len), kvp,
                                   H, Hkv, past_len, 64, spt, 128, BASE, 8192, True, int4, True)
parents = [-1, 0, 0] * B                                  # a fork: node 2 must not see node 1
cu_np, past_np = np.array([0, n, 2 * n], np.int32), np.array([past_len] * B, np.int32)
masks = A.tree_masks_from_parents(parents, cu_np).to(gpu)
qkv = dev(r.standard_normal((B * n, W)).astype(np.float16))
cu_q, past = dev(cu_np), dev(past_np)
A.append_tree_rope_update_kv_cache(qkv, cu_q, past, kvp, masks, H, Hkv, spt, BASE, int4)
out = torch.zeros((B * n, H, 128), dtype=torch.float16, device=gpu)
torch.cuda.synchronize()
g = torch.cuda.CUDAGraph()
with torch.cuda.graph(g):        # the FIRST split call of this process: no workspace yet, none may be allocated here
    A.append_tree_attention(qkv, cu_q, past, kvp, masks, H, Hkv, spt, int4, max_seqlen_q=n, out=out, max_past=past_len, num_splits=3)
g.replay()
torch.cuda.synchronize()
hp = host_pool(pools.k.cpu().numpy(), pools.v.cpu().numpy(), Hkv, int4)
ref = expected_tree(qkv.cpu().numpy(), cu_np, past_np, tables, hp, H, Hkv, words_from_parents(parents[:n]) * B)
err = float(np.abs(out.cpu().numpy().astype(np.float64) - ref).max())
same = torch.equal(out, A.append_tree_attention(qkv, cu_q, past, kvp, masks, H, Hkv, spt, int4, max_seqlen_q=n))
print(f"CHILD err={err:.3e} unsplit={int(same)}")
"""


def test_first_split_call_inside_a_capture_is_the_unsplit_tree_launch(gpu):
    """tests/test_append_split_gpu.py's rule for this entry's own fall-back, in a fresh process (the workspace is allocated lazily, once
    per process and device): B = 2, past 200 (4 pages), n = 3, a forking tree, 3 splits asked for."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _CHILD, root, os.path.join(root, "tests")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("CHILD")][-1]
    print(line)
    err, same = float(line.split("err=")[1].split()[0]), line.endswith("unsplit=1")
    assert err <= TOL, line
    assert same, "a first split call inside a capture must be the un-split tree launch, bit for bit"


# ---- 3. every mask bit ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("int4", KV)
@pytest.mark.parametrize("H,Hkv", [(4, 4), (3, 1)])
def test_every_mask_bit_is_honoured(gpu, H, Hkv, int4):
    """Attention only, on rows taken as already rotated; the words are random 64-bit values - own bit set or not, keys above the
    row, no closure -, so every (lane half, key block, register) position of the mask is hit with both values, through the row map of
    G = 1 and of G = 3 (where the rows of a wave straddle tokens).  Some words are all zero: at past 0 those rows are exactly 0."""
    from qserve_amd import append as A
    c = _Case(gpu, H, Hkv, int4, [0, 5], [64, 64], seed=29 * H + int(int4))
    words = [int(x) for x in c.r.integers(0, 2 ** 64, size=c.T, dtype=np.uint64)]
    empty = [3, 17, 40, 63, 64 + 9]
    for t in empty:
        words[t] = 0
    words[5], words[64 + 5] = 2 ** 64 - 1, 2 ** 64 - 1
    qkv = dev(c.new)
    ref = expected_tree(c.new, c.cu_q, c.past, c.tables, c.host(), H, Hkv, words)
    for splits in (1, 2):
        out = A.append_tree_attention(qkv, dev(c.cu_q), dev(c.past), c.kvp, dev(as_int64(words)), H, Hkv, c.spt, int4, max_seqlen_q=64,
                                      num_splits=splits)
        torch.cuda.synchronize()
        got = _np(out).astype(np.float64)
        err = np.abs(got - ref).max()
        print(f"every mask bit H={H} Hkv={Hkv} int4={int4} splits={splits}: max abs err {err:.3e}")
        assert np.isfinite(got).all() and err <= TOL, f"max abs err {err:.2e}"
        assert not got[[t for t in empty if t < 64]].any(), "a row that sees no key must be exactly 0"
        assert np.abs(got[64 + 9]).max() > 0                     # (an empty word over a past still sees the past)


# ---- 4. leaks -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("int4", KV)
@pytest.mark.parametrize("sibling", [2, 6], ids=["below", "above"])
def test_an_invisible_sibling_does_not_leak(gpu, sibling, int4):
    """Row 4 does not see node `sibling`, whose key is 8 x the row's query (a score of ~ 8 |q|^2 / sqrt(128) ~ 90, far above every
    other) and whose value is 1000: a leak shows as an error of order 1000."""
    from qserve_amd import append as A
    H = Hkv = 2
    row, n = 4, 8
    c = _Case(gpu, H, Hkv, int4, [5], [n], seed=41 + sibling)
    new = c.new.copy()
    new[sibling, H * 128:(H + Hkv) * 128] = 8 * new[row, : H * 128]
    new[sibling, (H + Hkv) * 128:] = 1000
    words = chain_words(n)
    words[row] &= ~(1 << sibling)
    assert not (words[row] >> sibling) & 1
    ref = expected_tree(new, c.cu_q, c.past, c.tables, c.host(), H, Hkv, words)
    out = A.append_tree_attention(dev(new), dev(c.cu_q), dev(c.past), c.kvp, dev(as_int64(words)), H, Hkv, c.spt, int4, max_seqlen_q=n)
    torch.cuda.synchronize()
    got = _np(out).astype(np.float64)
    err = np.abs(got[row] - ref[row]).max()
    print(f"leak test sibling {sibling}: row {row} max abs err {err:.3e}, |ref| max {np.abs(ref[row]).max():.2f}")
    assert np.isfinite(got).all() and err <= TOL
    leaky = list(words)
    leaky[row] |= 1 << sibling                                   # (the plant is live: seen, it would dominate the row)
    assert np.abs(expected_tree(new, c.cu_q, c.past, c.tables, c.host(), H, Hkv, leaky)[row]).min() > 900


# ---- 5. path commit -------------------------------------------------------------------------------------------------------------
def _tree_through(path, n, rng):
    """Parents of an n-node tree in which `path` (increasing node indices) is a chain hanging off the context - depth(path[k]) = k -
    and every other node hangs off a random earlier node or the context."""
    par = [(-1 if i == 0 or rng.random() < 0.3 else int(rng.integers(0, i))) for i in range(n)]
    for k, i in enumerate(path):
        par[i] = -1 if k == 0 else path[k - 1]
    return par


@pytest.mark.parametrize("pairing", [0, 1])
@pytest.mark.parametrize("int4", KV)
@pytest.mark.parametrize("H,Hkv", [(8, 2), (4, 4)])
def test_commit_path_moves_the_accepted_path_and_nothing_else(gpu, H, Hkv, int4, pairing):
    from qserve_amd import append as A
    from qserve_backend import fused_attention as fa
    n, pasts = 64, [0, 60, 63, 130]
    c = _Case(gpu, H, Hkv, int4, pasts, [n] * 4, seed=5 * H + Hkv + int(int4) + 100 * pairing, extra_blocks=2)
    rnd = sorted(c.r.choice(n, size=23, replace=False).tolist())
    lists = [[0, 1, 2], list(range(1, 64)), rnd, []]            # identity, the shift (every source the next move's destination), random, empty
    lists = lists[-pairing:] + lists[:-pairing] if pairing else lists
    B = len(pasts)
    parents = [p for b in range(B) for p in _tree_through(lists[b], n, c.r)]
    words = [w for b in range(B) for w in words_from_parents(parents[b * n:(b + 1) * n])]
    for b in range(B):
        assert [depths(words[b * n:(b + 1) * n], n)[i] for i in lists[b]] == list(range(len(lists[b])))
    cu_q, past = dev(c.cu_q), dev(c.past)
    start = c.clone_pools()                                      # the cache before the tree
    qkv = dev(c.new)
    A.append_tree_rope_update_kv_cache(qkv, cu_q, past, c.kvp, A.tree_masks_from_parents(parents, c.cu_q).to(gpu), H, Hkv, c.spt, BASE, int4)
    torch.cuda.synchronize()
    before = c.host()
    m = [len(x) for x in lists]
    idx = np.zeros((B, n), np.int32)
    for b in range(B):
        idx[b, : m[b]] = lists[b]
    A.commit_path(c.kvp, past, dev(idx), dev(np.asarray(m, np.int32)), Hkv, c.spt, int4)
    torch.cuda.synchronize()
    after = c.host()
    # the reference: the accepted rows' RAW qkv, in path order, through the linear writer over the cache before the tree
    rows = np.concatenate([b * n + np.asarray(lists[b], np.int64) for b in range(B)]).astype(np.int64)
    cu_m = np.concatenate([[0], np.cumsum(m)]).astype(np.int32)
    A.append_rope_update_kv_cache(dev(c.new[rows]), dev(cu_m), past, start.pointers(c.tables), H, Hkv, c.spt, BASE, int4)
    torch.cuda.synchronize()
    lin = c.host(start)
    # expected image: everything as before the commit, slots past .. past + m - 1 as the linear writer leaves them
    exp = copy.deepcopy(before)
    for b in range(B):
        for k in range(m[b]):
            pos = pasts[b] + k
            for which, (e_pool, l_pool) in enumerate(((exp.k, lin.k), (exp.v, lin.v))):
                blk = c.tables[b, which, pos // 64]
                for dst, src in zip(exp._views(e_pool, blk), lin._views(l_pool, blk)):
                    dst[:, pos % 64] = src[:, pos % 64]
    assert np.array_equal(after.k, exp.k), "K pages: a slot of the path differs from the linear writer's, or another byte changed"
    assert np.array_equal(after.v, exp.v), "V pages: a slot of the path differs from the linear writer's, or another byte changed"
    if any(lists[b] != list(range(m[b])) for b in range(B)):
        assert not np.array_equal(after.k, before.k)             # (the commit did move something)
    _spare_blocks_untouched(c.pools, c.tables, c.nblocks)
    # decode over the committed cache: the existing bar of single_query_attention (tests/test_attention_gpu.py) - 1e-3 against the
    # exact-de-quantisation oracle on contexts >= 64, the envelope of the oracle's three modes + 1e-3 on shorter ones
    lengths = (c.past + np.asarray(m, np.int32) + 1).astype(np.int32)
    one = c.r.standard_normal((B, c.W)).astype(np.float16)
    q, k, v = (x.reshape(B, -1, 128) for x in np.split(one, [H * 128, (H + Hkv) * 128], axis=1))
    x = dev(one)
    dq, dk, dv = x.split([H * 128, Hkv * 128, Hkv * 128], dim=-1)
    out = fa.single_query_attention(dq.reshape(B, H, 128), dk.reshape(B, Hkv, 128), dv.reshape(B, Hkv, 128), c.kvp, dev(lengths), None, 8192,
                                    64, c.spt, int(lengths.max()), 128, BASE, True, int4, True)
    torch.cuda.synchronize()
    o = _np(out).astype(np.float32)
    refs = np.stack([kvattn.decode_attention(q, k, v, c.tables, lengths, copy.deepcopy(after), BASE, mode).astype(np.float32)
                     for mode in ("kernel", "fp32", "exact")])
    env = refs.max(0) - refs.min(0) + 1e-3
    assert np.isfinite(o).all() and all((np.abs(o - r_) <= env).all() for r_ in refs), "decode over the committed cache: outside the envelope"
    long_rows = lengths >= 64
    err = np.abs(o - refs[2])[long_rows].max()
    print(f"decode over the committed cache: max abs err vs the exact oracle on contexts >= 64: {err:.3e}")
    assert err <= 1e-3


# ---- 6. the engine --------------------------------------------------------------------------------------------------------------
# Top-2 logit margin above which a drafted greedy token MUST be accepted.  The issue's rule: twice the largest logit difference
# observed between verify_tree and step() on the same positions - measured below against the reference engine (the test prints it
# on every run: "largest logit difference").  Recorded on the MI355X with TINY, B = 3, P = 70, seed 5: 2.5879e-02; twice that:
ENGINE_MARGIN = 5.1758e-2


def _greedy_rule_holds(par, toks, idx, lens, am):
    """Per sequence: the path starts at the root, every step goes to the FIRST child whose token is its parent's argmax, and no
    child of the last node matches."""
    n = len(par)
    for b in range(len(lens)):
        path = idx[b][: lens[b]]
        assert lens[b] >= 1 and path[0] == 0
        for a, c_ in zip(path, path[1:]):
            first = next(ch for ch in range(1, n) if par[ch] == a and toks[b][ch] == am[b][a])
            assert c_ == first
        assert not [ch for ch in range(1, n) if par[ch] == path[-1] and toks[b][ch] == am[b][path[-1]]]


def test_engine_verify_tree(gpu):
    """verify_tree over a 12-node tree that holds the greedy continuation g_1 .. g_4 of a reference engine plus random siblings.

    Largest logit difference between verify_tree and step() on the same positions, measured on the MI355X (TINY, B = 3, P = 70,
    seed 5): 2.5879e-02, printed again by every run; ENGINE_MARGIN is twice that figure."""
    import qserve_backend.layernorm_ops as layernorm_ops
    from qserve_amd.decode import TINY, DecodeEngine
    B, P, V = 3, 70, TINY["vocab"]
    toks = torch.randint(0, V, (B * P,), device=gpu, generator=torch.Generator(device=gpu).manual_seed(1))

    def engine():
        e = DecodeEngine(TINY, batch=B, prompt_len=P, max_new=40, device="cuda:0", seed=5)
        e.prefill(P, toks)
        return e

    # the reference: four decode steps; g[k] = token AFTER k + 1 steps, step_logits[k] = the logits that chose it
    ref = engine()
    root = ref.tokens.clone()
    g, step_logits = [], []
    for _ in range(4):
        ref.step()
        step_logits.append(torch.matmul(ref.final, ref.lm_head.t()).float())
        g.append(ref.tokens.clone())
    torch.cuda.synchronize()
    # the tree: nodes 1, 4, 7, 10 hold g_1 .. g_4 as a chain off the root; the others are random siblings
    par = [-1, 0, 0, 0, 1, 1, 2, 4, 4, 5, 7, 7]
    chain = [1, 4, 7, 10]
    n = len(par)
    r = np.random.default_rng(3)
    draft = torch.from_numpy(r.integers(0, V, size=(B, n))).to(gpu)
    for k, node in enumerate(chain):
        draft[:, node] = g[k]
        for sib in [c_ for c_ in range(n) if par[c_] == par[node] and c_ != node]:      # a sibling never holds the greedy token too
            draft[:, sib] = (g[k] + 1 + sib) % V
    eng = engine()
    assert torch.equal(eng.tokens, root)
    len0 = eng.lengths.clone()
    idx, lens, am = eng.verify_tree(draft, par)
    torch.cuda.synchronize()
    idx_h, lens_h, am_h = idx.tolist(), lens.tolist(), am.tolist()
    full = draft.clone()
    full[:, 0] = root
    _greedy_rule_holds(par, full.tolist(), idx_h, lens_h, am_h)
    assert torch.equal(eng.lengths, len0 + lens)
    assert eng.tokens.tolist() == [am_h[b][idx_h[b][lens_h[b] - 1]] for b in range(B)]
    # the logits of verify_tree at the chain's nodes against step()'s at the same positions
    vl = eng.last_verify_logits.float()
    nodes = [0] + chain[:3]
    diff = max((vl[:, node] - step_logits[k]).abs().max().item() for k, node in enumerate(nodes))
    sl = torch.stack(step_logits)                                        # [4, B, V]
    top2 = sl.topk(2, dim=-1).values
    margin = (top2[..., 0] - top2[..., 1])                               # [4, B]
    print(f"engine: largest logit difference between verify_tree and step() on the same positions {diff:.4e}; "
          f"top-2 margins of the greedy steps min {margin.min().item():.4e}")
    # layer-0 pages of the accepted slots against an engine that appended the accepted tokens linearly (layer 0 is per-row
    # deterministic: embedding, norm + quant, qkv GEMM, writer)
    from qserve_amd import append as A
    lin = engine()
    acc = [[int(full[b, i]) for i in idx_h[b][: lens_h[b]]] for b in range(B)]
    m = lens_h
    cu = torch.tensor(np.concatenate([[0], np.cumsum(m)]), dtype=torch.int32, device=gpu)
    past = (len0 - 1).to(torch.int32)
    h = torch.index_select(lin.embed, 0, torch.tensor([t for a in acc for t in a], device=gpu))

    def attend(li, qkv):
        return A.append(qkv, cu, past, lin.tables[li], lin.H, lin.Hkv, lin.size_per_token, TINY["rope_theta"], lin.int4,
                        max_seqlen_q=max(m)).reshape(sum(m), -1)

    lin._prompt_layers(h, lin._prompt_buffers(sum(m)), attend)
    torch.cuda.synchronize()
    hp_e = host_pool(_np(eng.pools[0][0]), _np(eng.pools[0][1]), eng.Hkv, True)
    hp_l = host_pool(_np(lin.pools[0][0]), _np(lin.pools[0][1]), lin.Hkv, True)
    tab = ((_np(eng.tables[0]) - np.array([eng.pools[0][0].data_ptr(), eng.pools[0][1].data_ptr()])[None, :, None]) // eng.page_bytes)
    for b in range(B):
        L = int(past[b]) + m[b]
        for which in ("k", "v"):
            for hd in range(eng.Hkv):
                e_ = hp_e.read_tokens(which, tab[b, 0 if which == "k" else 1], hd, L)
                l_ = hp_l.read_tokens(which, tab[b, 0 if which == "k" else 1], hd, L)
                assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(e_, l_)), f"layer-0 {which} pages differ"
    # the engine goes on: capture, two replays
    eng.capture()
    eng.run()
    eng.run()
    torch.cuda.synchronize()
    eng.check()
    assert torch.equal(eng.lengths, len0 + lens + 3)                     # capture() ran one warm-up step, then two replays
    assert bool(((eng.tokens >= 0) & (eng.tokens < V)).all()) and bool(torch.isfinite(eng.hidden).all())
    # a second verify_tree, now on ragged lengths
    draft2 = torch.from_numpy(r.integers(0, V, size=(B, n))).to(gpu)
    root2, len1 = eng.tokens.clone(), eng.lengths.clone()
    k0, v0 = eng.pools[0][0].clone(), eng.pools[0][1].clone()
    idx2, lens2, am2 = eng.verify_tree(draft2, par)
    torch.cuda.synchronize()
    full2 = draft2.clone()
    full2[:, 0] = root2
    _greedy_rule_holds(par, full2.tolist(), idx2.tolist(), lens2.tolist(), am2.tolist())
    assert torch.equal(eng.lengths, len1 + lens2)
    assert eng.tokens.tolist() == [am2.tolist()[b][idx2.tolist()[b][lens2.tolist()[b] - 1]] for b in range(B)]
    # layer-0 pages again: the accepted tokens through the second engine's layer-0 ops (same seed: same weights) and the linear
    # writer, into copies of the pages as they were before this call
    m2 = lens2.tolist()
    acc2 = torch.tensor([int(full2[b, i]) for b in range(B) for i in idx2.tolist()[b][: m2[b]]], device=gpu)
    h2 = torch.index_select(lin.embed, 0, acc2)
    bufs = lin._prompt_buffers(sum(m2))
    layernorm_ops.rms_norm_general_fuse_sum(bufs["qa"], h2, lin.layers[0]["ln1"], bufs["q_sum"], bufs["q_scale"], TINY["eps"], True)
    lin.layers[0]["qkv"](bufs["qa"], bufs["q_scale"], bufs["q_sum"], bufs["qkv"])
    moved = eng.tables[0].clone()
    moved[:, 0] += k0.data_ptr() - eng.pools[0][0].data_ptr()
    moved[:, 1] += v0.data_ptr() - eng.pools[0][1].data_ptr()
    cu2 = torch.tensor(np.concatenate([[0], np.cumsum(m2)]), dtype=torch.int32, device=gpu)
    A.append_rope_update_kv_cache(bufs["qkv"], cu2, (len1 - 1).to(torch.int32), moved, lin.H, lin.Hkv, lin.size_per_token, TINY["rope_theta"],
                                  lin.int4)
    torch.cuda.synchronize()
    hp_e, hp_l = host_pool(_np(eng.pools[0][0]), _np(eng.pools[0][1]), eng.Hkv, True), host_pool(_np(k0), _np(v0), eng.Hkv, True)
    for b in range(B):
        L = int(len1[b]) - 1 + m2[b]
        for which in ("k", "v"):
            for hd in range(eng.Hkv):
                e_ = hp_e.read_tokens(which, tab[b, 0 if which == "k" else 1], hd, L)
                l_ = hp_l.read_tokens(which, tab[b, 0 if which == "k" else 1], hd, L)
                assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(e_, l_)), f"second call: layer-0 {which} pages differ"
    eng.step()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(eng.final.float()).all())
    # the drafted greedy tokens must have been accepted wherever the reference's own top-2 margin is beyond the numerical difference
    for b in range(B):
        for k, node in enumerate(chain):
            if all(margin[j, b].item() > ENGINE_MARGIN for j in range(k + 1)):
                assert lens_h[b] > k + 1 and idx_h[b][k + 1] == node, f"sequence {b}: g_{k + 1} not accepted at a margin {margin[k, b].item():.3e}"
