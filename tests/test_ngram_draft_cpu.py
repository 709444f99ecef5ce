"""The n-gram tree drafter without a GPU: the numpy reference of tests/_draft_cases.py against hand-worked cases and against a literal
loop-by-loop reading of the rule, `qs_ngram_draft_tree` / `qs_history_append`'s argument validation (which happens before any HIP call),
and the argument checks of qserve_amd.drafting."""
import numpy as np
import pytest
import torch

from _draft_cases import MALFORMED, NGRAMS, TREES, chain, reference_append, reference_draft, star

PAD = -1


def _literal(h, parents, max_ngram, min_match, pad):
    """The rule of include/qserve_amd.h word for word, in plain Python (slow: small cases only)."""
    h = [int(x) for x in h]
    L, n = len(h), len(parents)
    draft, path = [h[-1] if L else pad], {0: []}
    for i in range(1, n):
        a = parents[i]
        if not 0 <= a < i:
            draft.append(pad)
            path[i] = [pad]
            continue
        c = h + path[a]
        used = {draft[s] for s in range(1, i) if parents[s] == a}
        best = None
        for p in range(1, L):
            m = 0
            while m < min(max_ngram, p) and h[p - 1 - m] == c[len(c) - 1 - m]:
                m += 1
            if m >= min_match and h[p] not in used and (best is None or (m, p) > best):
                best = (m, p)
        draft.append(h[best[1]] if best else pad)
        path[i] = path[a] + [draft[i]]
    return draft


def test_a_periodic_history_continues_its_period_along_a_chain():
    h = [1, 2, 3, 4] * 3 + [1, 2]                                   # ... 3 4 1 2 | the period goes on with 3 4 1 2 3
    assert reference_draft(h, len(h), chain(6), 4, 1, PAD) == [2, 3, 4, 1, 2, 3]
    assert reference_draft(h, len(h), chain(6), 16, 2, PAD) == [2, 3, 4, 1, 2, 3]
    # what lies behind the length is not read: the same history with a tail of other tokens
    assert reference_draft(h + [9, 9, 2, 7], len(h), chain(6), 4, 1, PAD) == [2, 3, 4, 1, 2, 3]


def test_star_siblings_are_distinct_and_ranked_longest_then_latest():
    #    p:  0  1  2  3  4  5  6  7  8  9
    h = [5, 7, 1, 7, 2, 5, 7, 3, 6, 7]
    # the root is 7 and c ends "6 7".  7 is followed by something at p = 2, 4 and 7; before it stands 5, 1 and 5, never 6, so m = 1
    # everywhere and recency ranks the candidates: h[7] = 3, h[4] = 2, h[2] = 1, then none.
    assert reference_draft(h, len(h), star(5), 4, 1, PAD) == [7, 3, 2, 1, PAD]
    # a longer match beats a later one: "6 7" stands before p = 5, a 2-gram match
    h2 = [5, 7, 1, 6, 7, 2, 5, 7, 3, 6, 7]
    assert reference_draft(h2, len(h2), star(5), 4, 1, PAD) == [7, 2, 3, 1, PAD]
    # equal continuations are proposed once: 7 is followed by 3 twice and by 1 once
    h3 = [7, 3, 7, 1, 7, 3, 0, 7]
    assert reference_draft(h3, len(h3), star(4), 4, 1, PAD) == [7, 3, 1, PAD]


def test_lengths_zero_and_one_give_pad():
    for par in (chain(4), star(4), TREES["par12"]):
        n = len(par)
        assert reference_draft([3, 3, 3], 0, par, 4, 1, PAD) == [PAD] * n
        assert reference_draft([3, 3, 3], 1, par, 4, 1, PAD) == [3] + [PAD] * (n - 1)
    assert reference_draft([3, 3, 3], 2, chain(3), 4, 1, PAD) == [3, 3, 3]       # L = 2: p = 1 matches h[0], then the drafted 3 matches too


def test_min_match_two_rejects_one_gram_matches():
    h = [4, 8, 1, 9, 8]                                               # 8 occurs before (followed by 1), but "9 8" does not
    assert reference_draft(h, len(h), chain(3), 4, 1, PAD) == [8, 1, 9]
    assert reference_draft(h, len(h), chain(3), 4, 2, PAD) == [8, PAD, PAD]
    h = [9, 8, 1, 9, 8]                                               # now "9 8" does
    assert reference_draft(h, len(h), chain(3), 4, 2, PAD) == [8, 1, 9]


def test_max_ngram_one_is_pure_recency():
    h = [6, 7, 1, 5, 7, 2, 6, 7]                                      # "6 7" -> 1 is the longer match, "7" -> 2 the later one
    assert reference_draft(h, len(h), chain(2), 4, 1, PAD) == [7, 1]
    assert reference_draft(h, len(h), chain(2), 1, 1, PAD) == [7, 2]


def test_exhausted_exclusion_gives_pad_and_a_pad_nodes_child_follows_the_rule():
    h = [2, 5, 2, 5, 2]                                               # 2 is only ever followed by 5
    par = [-1, 0, 0, 2, 1]                                            # node 2 finds nothing new; node 3 hangs off that pad node
    got = reference_draft(h, len(h), par, 4, 1, PAD)
    assert got[:3] == [2, 5, PAD]
    assert got[3] == PAD                                              # c = h + [PAD]: PAD occurs nowhere in h
    assert got[4] == 2                                                # c = h + [5]: "2 5" -> 2
    # pad is a token like any other: with pad = 5 the child of the pad node continues "2 5" with 2
    assert reference_draft(h, len(h), par, 4, 1, 5) == [2, 5, 5, 2, 2]


def test_malformed_parents_take_pad_and_their_children_follow_the_rule():
    h = [1, 2, 3, 1, 2, 3, 1]
    got = reference_draft(h, len(h), MALFORMED, 4, 1, 2)
    for i, a in enumerate(MALFORMED):
        if i and not 0 <= a < i:
            assert got[i] == 2, f"node {i}"
    # node 7 hangs off node 6 (malformed, pad = 2): its c is h + [2], and "1 2" goes on with 3
    assert MALFORMED[7] == 6 and got[7] == 3


def test_the_reference_is_the_literal_rule_on_random_cases():
    rng = np.random.default_rng(4)
    trees = list(TREES.values()) + [MALFORMED]
    longest = 0
    for case in range(300):
        par = trees[case % len(trees)]
        L = int(rng.integers(0, 40))
        h = rng.integers(0, int(rng.choice([2, 5, 50])), size=L + 3)
        mx, mn = NGRAMS[int(rng.integers(0, len(NGRAMS)))]
        pad = int(rng.choice([PAD, 0, 1 << 40]))
        got = reference_draft(h, L, par, mx, mn, pad)
        assert got == _literal(h[:L], par, mx, mn, pad), f"case {case}"
        longest = max(longest, sum(t != pad for t in got))
    assert longest >= 12, "no case drafted more than a few nodes"


def test_reference_append():
    hist = np.arange(20, dtype=np.int32).reshape(2, 10) + 100
    nodes = np.array([[50, 51, 52, 53], [60, 61, 62, 63]])
    idx = np.array([[0, 2, 3, 0], [0, 1, 0, 0]], np.int32)
    out = reference_append(hist, [3, 7], nodes, idx, [3, 2], [77, 88])
    want = hist.copy()
    want[0, 4:7] = [52, 53, 77]
    want[1, 8:10] = [61, 88]
    assert np.array_equal(out, want)
    out = reference_append(hist, [3, 8], nodes, idx, [1, 2], [77, 88])        # the bonus token alone; a row clipped at cap
    want = hist.copy()
    want[0, 4] = 77
    want[1, 9] = 61
    assert np.array_equal(out, want)


def test_argument_validation_without_gpu(built_lib):
    from qserve_amd._lib import lib

    def draft(history=4096, stride=64, cap=64, lengths=8192, parents=12288, batch=2, n=12, max_ngram=4, min_match=1, out=16384):
        return lib.qs_ngram_draft_tree(history, stride, cap, lengths, parents, batch, n, max_ngram, min_match, 0, out, None)

    for bad in ("history", "lengths", "parents", "out"):
        assert draft(**{bad: None}) == -1 and b"null pointer" in lib.qs_last_error(), bad
    assert draft(n=0) == -1 and b"n=0" in lib.qs_last_error()
    assert draft(n=65) == -1 and b"n=65" in lib.qs_last_error()
    assert draft(max_ngram=0) == -1 and draft(max_ngram=17) == -1 and b"max_ngram=17" in lib.qs_last_error()
    assert draft(min_match=0) == -1 and draft(max_ngram=3, min_match=4) == -1 and b"min_match=4" in lib.qs_last_error()
    assert draft(cap=0) == -1 and b"cap=0" in lib.qs_last_error()
    assert draft(stride=63) == -1 and b"hist_stride=63" in lib.qs_last_error()
    assert draft(batch=-1) == -1
    assert draft(batch=0) == 0                                               # nothing to do: no launch

    def append(history=4096, stride=64, cap=64, past=8192, nodes=12288, idx=16384, lens=20480, nxt=24576, batch=2, n=12, max_accept=12):
        return lib.qs_history_append(history, stride, cap, past, nodes, idx, lens, nxt, batch, n, max_accept, None)

    for bad in ("history", "past", "nodes", "idx", "lens", "nxt"):
        assert append(**{bad: None}) == -1 and b"null pointer" in lib.qs_last_error(), bad
    assert append(n=0) == -1 and append(n=65) == -1 and b"n=65" in lib.qs_last_error()
    assert append(max_accept=0) == -1 and append(max_accept=65) == -1 and b"max_accept=65" in lib.qs_last_error()
    assert append(cap=0) == -1 and append(stride=10) == -1 and b"hist_stride=10" in lib.qs_last_error()
    assert append(batch=-1) == -1
    assert append(batch=0) == 0
    assert lib.qs_ngram_draft_lds_tokens() >= 8192


def test_drafting_argument_checks(built_lib):
    """Wrong dtypes and shapes are reported with the argument's name before anything is launched (CPU tensors: the device check
    comes last)."""
    from qserve_amd import drafting as D
    assert D.LDS_TOKENS == D.lib.qs_ngram_draft_lds_tokens()
    hist, lens, par = torch.zeros((3, 16), dtype=torch.int32), torch.zeros((3,), dtype=torch.int32), torch.tensor([-1, 0], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="history"):
        D.ngram_draft_tree(hist.long(), lens, par)
    with pytest.raises(RuntimeError, match="history must be"):
        D.ngram_draft_tree(hist[0], lens, par)
    with pytest.raises(RuntimeError, match="history must be"):
        D.ngram_draft_tree(hist.t(), lens, par)                              # no unit column stride
    with pytest.raises(RuntimeError, match="lengths"):
        D.ngram_draft_tree(hist, lens.long(), par)
    with pytest.raises(RuntimeError, match="lengths must be"):
        D.ngram_draft_tree(hist, lens[:2], par)
    with pytest.raises(RuntimeError, match="parents"):
        D.ngram_draft_tree(hist, lens, par.long())
    with pytest.raises(RuntimeError, match="parents must be"):
        D.ngram_draft_tree(hist, lens, torch.zeros((65,), dtype=torch.int32))
    with pytest.raises(RuntimeError, match="history must be on CUDA"):
        D.ngram_draft_tree(hist, lens, par)                                  # everything else is right: the device is what is left
    nodes, idx, nxt = torch.zeros((3, 2), dtype=torch.int64), torch.zeros((3, 2), dtype=torch.int32), torch.zeros((3,), dtype=torch.int64)
    with pytest.raises(RuntimeError, match="node_tokens"):
        D.history_append(hist, lens, nodes.int(), idx, lens, nxt)
    with pytest.raises(RuntimeError, match="accept_idx must be"):
        D.history_append(hist, lens, nodes, idx[:2], lens, nxt)
    with pytest.raises(RuntimeError, match="next_token"):
        D.history_append(hist, lens, nodes, idx, lens, nxt.int())
    with pytest.raises(RuntimeError, match="past_lens must be"):
        D.history_append(hist, lens.view(3, 1), nodes, idx, lens, nxt)
