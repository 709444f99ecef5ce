"""Expected values of the n-gram tree drafter and of the history append (qs_ngram_draft_tree, qs_history_append;
qserve_amd.drafting; DecodeEngine.draft_tree / speculate): the rule of include/qserve_amd.h restated in numpy, and the trees and
histories the CPU and the GPU tests share.  The product does not import this file.

The rule, for one sequence.  h = history[:L]; node 0 carries h[L-1] (pad if L == 0).  Node i >= 1 with parent a: c = h followed by the
draft tokens on the path root -> a without the root's own; for a history position 1 <= p <= L-1 the match length m(p) is the largest
m <= min(max_ngram, p) with h[p-1-j] == c[len(c)-1-j] for all j < m; p is a candidate if m(p) >= min_match and h[p] is the token of no
earlier sibling; the node takes h[p*] of the candidate with the largest (m(p), p), or pad if there is none.  A node whose parent entry
is not in 0 .. i-1 takes pad, and its path is the node alone."""
import numpy as np

PAR12 = [-1, 0, 0, 0, 1, 1, 2, 4, 4, 5, 7, 7]            # the 12-node tree of tests/_accept_engine.py (PAR)


def chain(n):
    return [-1] + list(range(n - 1))


def star(n):
    return [-1] + [0] * (n - 1)


def tree64(seed=2):
    """64 nodes: a random tree with a wide root (8 children, so exclusion lists outgrow a vocabulary of 5) and random deeper nodes."""
    rng = np.random.default_rng(seed)
    return [-1] + [0] * 8 + [int(rng.integers(0, i)) for i in range(9, 64)]


TREES = {"chain5": chain(5), "star6": star(6), "par12": PAR12, "tree64": tree64(), "root": [-1]}
NGRAMS = [(1, 1), (3, 1), (3, 2), (16, 1), (16, 2)]      # (max_ngram, min_match)
# parents no tree has (the values the header defines: such a node takes pad, its path is the node alone, its children follow the rule)
MALFORMED = [-1, 0, 5, 2, -3, 1, 64, 6, 4, 8, 1 << 30, 10]


def reference_draft(history, L, parents, max_ngram=4, min_match=1, pad=0):
    """-> the n drafted tokens (python ints) of one sequence: history[:min(L, len(history))] is its text."""
    h = np.asarray(history, np.int64)[:max(0, min(int(L), len(history)))]
    L, n = len(h), len(parents)
    draft = [int(h[-1]) if L else int(pad)]
    path = [[]]                                           # per node: the draft tokens root -> node, the root's excluded
    p = np.arange(1, L)
    for i in range(1, n):
        a = int(parents[i])
        if not 0 <= a < i:
            draft.append(int(pad))
            path.append([int(pad)])
            continue
        c = np.concatenate([h, np.asarray(path[a], np.int64)])
        m, alive = np.zeros(p.shape, np.int64), np.ones(p.shape, bool)
        for j in range(max_ngram):                        # m(p): how many of h[p-1], h[p-2], ... agree with c[-1], c[-2], ... (j < p)
            alive = alive & (p - 1 - j >= 0)
            if not alive.any():                           # (also: no p left means c may be shorter than j + 1)
                break
            alive[alive] = h[p[alive] - 1 - j] == c[len(c) - 1 - j]
            m += alive
        used = [draft[s] for s in range(1, i) if int(parents[s]) == a]
        cand = (m >= min_match) & ~np.isin(h[p], np.asarray(used, np.int64))
        if cand.any():
            key = np.where(cand, m * (1 << 32) + p, -1)
            tok = int(h[int(key.max()) & 0xFFFFFFFF])
        else:
            tok = int(pad)
        draft.append(tok)
        path.append(path[a] + [tok])
    return draft


def reference_draft_batch(history, lengths, parents, max_ngram=4, min_match=1, pad=0):
    """history [B, cap], lengths [B] -> int64 [B, n]."""
    return np.array([reference_draft(history[b], lengths[b], parents, max_ngram, min_match, pad) for b in range(len(lengths))], np.int64)


def reference_append(history, past, node_tokens, accept_idx, accept_lens, next_token):
    """-> a copy of history [B, cap] with the accepted path (behind the root) and the bonus token recorded; writes beyond cap dropped."""
    out = np.array(history, copy=True)
    cap = out.shape[1]
    for b in range(out.shape[0]):
        m = int(accept_lens[b])
        vals = [int(node_tokens[b][int(accept_idx[b][j])]) for j in range(1, m)] + [int(next_token[b])]
        for j, v in enumerate(vals, start=1):
            if m >= 1 and 0 <= int(past[b]) + j < cap:
                out[b, int(past[b]) + j] = v
    return out


def small_histories(rng, cap, vocab, lengths):
    """history int32 [B, cap] of tokens below `vocab` (every column filled: what lies behind a sequence's length must not matter)."""
    return rng.integers(0, vocab, size=(len(lengths), cap)).astype(np.int32)
