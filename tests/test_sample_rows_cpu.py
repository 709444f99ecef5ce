"""The row sampler without a GPU: the float64 oracle against an independent sort-based restatement, the Philox known answer, the
losslessness of the keyed walk of sampled tree verification on a toy model, and `qs_sample_rows`'s argument validation (which happens
before any HIP call)."""
import ctypes

import numpy as np
import torch

from _sample_cases import Row, depths, philox4x32_10, philox_uniform, position_keys, walk


def _sorted_sampler(x, T, k, p, u):
    """What a sampler built from logits warpers does, in float64: temperature, sort, softmax, cumsum, nucleus cut in sorted order, then
    top-k on the filtered scores, then the draw over the renormalised survivors in index order -> (survivor mask, token)."""
    s = torch.from_numpy(x.astype(np.float64)) / float(np.float32(T))
    if float(np.float32(p)) < 1.0:
        srt, idx = torch.sort(s, descending=True)
        pr = torch.softmax(srt, dim=0)
        before = torch.cumsum(pr, dim=0) - pr                       # mass strictly in front of a sorted position
        drop = before >= float(np.float32(p))
        s = s.clone()
        s[idx[drop]] = -float("inf")
    if 0 < k < s.numel():
        kth = torch.topk(s, k).values[-1]
        s = torch.where(s < kth, torch.full_like(s, -float("inf")), s)
    keep = torch.isfinite(s)
    w = torch.where(keep, torch.exp(s - s.max()), torch.zeros_like(s))
    cum = torch.cumsum(w, dim=0)
    hit = torch.nonzero(keep & (cum > u * cum[-1]))
    tok = int(hit[0]) if hit.numel() else int(torch.nonzero(keep)[-1])
    return keep.numpy(), tok


def test_oracle_equals_a_sort_based_sampler_on_tie_free_rows():
    rng = np.random.default_rng(11)
    for case in range(1000):
        n = int(rng.integers(8, 200))
        # tie-free fp16 rows: distinct multiples of 1/16 below 2048 / 16 are exact in fp16
        x = (rng.permutation(2048)[:n].astype(np.float64) / 16.0 - 64.0).astype(np.float16)
        assert np.unique(x).size == n
        T = float(rng.choice([0.3, 0.8, 1.0, 2.5]))
        k = int(rng.choice([0, 1, 5, 50, n, n + 3]))
        p = float(rng.choice([0.1, 0.5, 0.9, 0.99, 1.0]))
        u = float(np.float32(rng.random()))
        row = Row(x, T, k, p)
        keep, tok = _sorted_sampler(x, T, k, p, u)
        assert np.array_equal(row.survivors(), keep), f"case {case}: survivor sets differ (n={n}, T={T}, k={k}, p={p})"
        assert row.token(u) == tok, f"case {case}: token {row.token(u)} != {tok} (n={n}, T={T}, k={k}, p={p}, u={u})"


def test_oracle_keeps_tie_classes_whole_and_masks_minus_inf():
    x = np.array([1, 3, 3, -np.inf, 2, 3, 0, 1], dtype=np.float16)
    row = Row(x, 1.0, 1, 1.0)                                        # top-1 with a three-way tie: all three stay
    assert row.survivors().tolist() == [False, True, True, False, False, True, False, False]
    assert [row.token(u) for u in (0.0, 0.34, 0.67, 1 - 2 ** -24)] == [1, 2, 5, 5]
    row = Row(x, 1.0, 0, 1e-6)                                       # a nucleus of (almost) nothing is the maximum's class
    assert row.survivors().sum() == 3
    assert Row(x, 1e-6, 0, 1.0).greedy and Row(x, 1.0, 0, 1e-9).greedy and Row(x, 1e-6).token(0.9) == 1
    row = Row(x, 1.0, 0, 1.0)
    assert all(row.token(u) != 3 for u in np.linspace(0, 1 - 2 ** -24, 97))


def test_philox_known_answer():
    """Random123's known-answer vectors for Philox4x32-10: the zero counter and key, and the all-ones counter and key."""
    out = philox4x32_10(np.zeros(4, dtype=np.uint32), np.zeros(2, dtype=np.uint32))
    assert [f"{int(v):08x}" for v in out] == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    out = philox4x32_10(np.full(4, 0xFFFFFFFF, dtype=np.uint32), np.full(2, 0xFFFFFFFF, dtype=np.uint32))
    assert [f"{int(v):08x}" for v in out] == ["408f276d", "41c83b0e", "a20bc7c6", "6d5451fd"]
    u = philox_uniform([0], 0)
    assert u.dtype == np.float32 and float(u[0]) == (0x6627e8d5 >> 8) * 2.0 ** -24


def test_position_keys_match_the_numpy_statement():
    from qserve_amd.sampling import position_keys as pk
    seq, pos = torch.tensor([0, 1, 2, 70000], dtype=torch.int32), torch.tensor([5, 0, 123456, 2 ** 31 - 1], dtype=torch.int32)
    got = pk(seq, pos)
    assert got.dtype == torch.int64 and got.tolist() == position_keys(seq.numpy(), pos.numpy()).tolist()


def _toy_logits(prefix, V):
    """A fixed table of logits per prefix: the row is a function of the prefix alone."""
    h = 1469598103934665603
    for t in prefix:
        h = ((h ^ (int(t) + 1)) * 1099511628211) % (1 << 64)
    return (np.random.default_rng(h).standard_normal(V) * 2.0).astype(np.float16)


def test_keyed_walk_is_lossless_on_a_toy_model():
    """Random trees and drafts over an exact toy model: the tokens the walk accepts, plus its bonus token, are the first tokens of the
    chain sampled sequentially with the same per-position keys - whatever was drafted."""
    rng = np.random.default_rng(5)
    V, seed = 12, 1234
    longest = 0
    for case in range(500):
        n = int(rng.integers(1, 17))
        par = [-1] + [int(rng.integers(0, i)) for i in range(1, n)]
        dep = depths(par)
        b = int(rng.integers(0, 8))
        ctx = rng.integers(0, V, size=int(rng.integers(1, 6))).tolist()      # the context; its last token is the root's
        T, k, p = float(rng.choice([0.7, 1.0, 1.5])), int(rng.choice([0, 3])), float(rng.choice([0.8, 1.0]))
        L = len(ctx)                                                        # `lengths`: the context including the root's token

        def draw(prefix, position):
            u = philox_uniform(position_keys([b], [position]), seed)[0]
            return Row(_toy_logits(prefix, V), T, k, p).token(u)

        # the sequential chain: the token at position L + j follows the prefix of L + j tokens
        chain, prefix = [], list(ctx)
        for j in range(n + 1):
            chain.append(draw(prefix, L + j))
            prefix.append(chain[-1])
        # the tree: node i carries draft[i] (the root the context's last token), its prefix is the context plus its ancestors' tokens
        draft = [ctx[-1]] + rng.integers(0, V, size=n - 1).tolist()
        if n > 1 and case % 2 == 0:                                         # half of the cases: plant the chain along one path
            i = 0
            for j in range(n):
                kids = [c for c in range(n) if par[c] == i]
                if not kids:
                    break
                i = kids[int(rng.integers(0, len(kids)))]
                draft[i] = chain[dep[i] - 1]
        sampled = []
        for i in range(n):
            anc, j = [], i
            while j > 0:
                anc.append(draft[j])
                j = par[j]
            sampled.append(draw(ctx + anc[::-1], L - 1 + dep[i] + 1))
        path, bonus = walk(par, draft, sampled)
        got = [draft[i] for i in path[1:]] + [bonus]
        assert got == chain[:len(got)], f"case {case}: walk {got}, chain {chain[:len(got)]}"
        longest = max(longest, len(path))
    assert longest >= 4, "no case accepted a path of depth 3: the walk was only checked near the root"


def test_argument_validation_without_gpu(built_lib):
    from qserve_amd._lib import lib

    def call(logits=4096, out=8192, rows=2, n=16, stride=16, row_keys=None, u_out=None):
        return lib.qs_sample_rows(logits, out, rows, n, stride, 1.0, 0, 1.0, None, None, None, None, 0, row_keys, u_out, None)

    assert call(logits=None) == -1 and b"null pointer" in lib.qs_last_error()
    assert call(out=None) == -1
    assert call(n=7, stride=8) == -1 and b"n=7" in lib.qs_last_error()
    assert call(n=16, stride=20) == -1                                       # a stride that is no multiple of 8
    assert call(n=24, stride=16) == -1                                       # a stride below n
    assert call(out=8196) == -1 and b"8-byte" in lib.qs_last_error()         # misaligned out
    assert call(logits=4104) == -1 and b"16-byte" in lib.qs_last_error()
    assert call(row_keys=8196) == -1 and call(u_out=8194) == -1
    assert call(rows=-1) == -1
    assert call(rows=0) == 0                                                 # nothing to do: no launch
    assert lib.qs_sample_rows.argtypes[12] is ctypes.c_uint64                # the seed: 64 unsigned bits
