"""Expected values of tree-draft verification: a float64 numpy attention with an ARBITRARY per-row visibility among the new tokens,
over the keys / values that tests/_append_cases.compose() builds (cached positions de-quantised with the kernels' values, the call's
own rotated k / raw v in fp16).  Row i of sequence b sees every cached key < past[b] and new key j iff j < n_b and bit j of its
64-bit word is set - the whole rule; nothing about j <= i or ancestor closure is assumed.  A row that sees no key is 0.

The arithmetic per (sequence, head) is oracle.flash.attention_varlen's, statement for statement, with the mask exchanged: with chain
words the two agree to the last bit (tests/test_append_tree_cpu.py pins that)."""
import numpy as np

from _append_cases import compose
from oracle import kvattn


def chain_words(n):
    return [(2 << i) - 1 for i in range(n)]


def words_from_parents(parents):
    """Ancestor-closed words (python ints) of ONE tree given as a parent list (-1: hangs off the context)."""
    w = []
    for i, p in enumerate(parents):
        assert -1 <= p < i
        w.append((w[p] if p >= 0 else 0) | (1 << i))
    return w


def random_parents(rng, n, roots=0.15):
    """A random forest in topological order: node i hangs off the context with probability `roots`, else off a random earlier node."""
    return [-1 if i == 0 or rng.random() < roots else int(rng.integers(0, i)) for i in range(n)]


def as_int64(words):
    """python ints (uint64 bit patterns) -> numpy int64 of the same bits (what the library reads as uint64)."""
    return np.array([int(w) & 0xFFFFFFFFFFFFFFFF for w in words], dtype=np.uint64).view(np.int64)


def depths(words, n):
    return [max(bin(int(w) & ((1 << n) - 1)).count("1") - 1, 0) for w in words]


def visibility(words, n):
    """bool [n, n]: vis[i, j] = bit j of word i (bits >= n dropped)."""
    return np.array([[(int(w) >> j) & 1 == 1 for j in range(n)] for w in words], dtype=bool).reshape(n, n)


def rotate_rows_tree(qkv, cu_q, past, words, H, Hkv, rope_base):
    """What the tree writer leaves in the packed buffer: q and k heads of node i of sequence b rotated at past[b] + depth(i)."""
    out = np.array(qkv, np.float16, copy=True)
    for b in range(len(past)):
        s, e = int(cu_q[b]), int(cu_q[b + 1])
        d = depths(words[s:e], e - s)
        for i, t in enumerate(range(s, e)):
            qk = out[t, : (H + Hkv) * 128].reshape(H + Hkv, 128)
            qk[:] = kvattn.rope_neox(qk, int(past[b]) + d[i], rope_base)
    return out


def expected_tree(qkv_rot, cu_q, past, tables, pool, H, Hkv, words):
    """float64 [T, H, 128]: tree attention of the already rotated rows over `pool` (only positions < past are read)."""
    q, k, v, cu_k = compose(qkv_rot, cu_q, past, tables, pool, H, Hkv)
    Tq, D = q.shape[0], q.shape[2]
    G = H // Hkv
    scale = 1.0 / np.sqrt(D)
    out = np.zeros((Tq, H, D), np.float64)
    for b in range(len(past)):
        qs, qe, ks, ke = int(cu_q[b]), int(cu_q[b + 1]), int(cu_k[b]), int(cu_k[b + 1])
        lq, lk, p = qe - qs, ke - ks, int(past[b])
        if lq == 0:
            continue
        vis = np.concatenate([np.ones((lq, p), bool), visibility(words[qs:qe], lq)], axis=1)
        assert vis.shape == (lq, lk)
        for h in range(H):
            Q = q[qs:qe, h].astype(np.float64)
            K = k[ks:ke, h // G].astype(np.float64)
            V = v[ks:ke, h // G].astype(np.float64)
            S = (Q @ K.T) * scale
            S = np.where(vis, S, -np.inf)
            m = S.max(axis=1, keepdims=True) if lk > 0 else np.zeros((lq, 1))
            m = np.where(np.isfinite(m), m, 0.0)
            P = np.exp(S - m)
            l = P.sum(axis=1, keepdims=True)
            out[qs:qe, h] = np.where(l > 0, (P @ V) / np.where(l > 0, l, 1.0), 0.0)
    return out
