"""GPU tests of the n-gram tree drafter and the history append (qserve_amd.drafting; csrc/ngram_draft.hip) against the numpy
restatement of tests/_draft_cases.py: exact integers, torch.equal, no tolerance."""
import numpy as np
import pytest
import torch

from _draft_cases import MALFORMED, NGRAMS, TREES, reference_append, reference_draft_batch
from _helpers import dev

pytestmark = pytest.mark.gpu
CAP, STRIDE = 50, 64                                     # hist_stride > cap: the rows are views into a wider buffer
LENGTHS = [[0, 37, CAP], [1, 2, 37]]                     # B = 3, ragged, all of {0, 1, 2, 37, cap}


def _padded(hist, stride):
    """The history as a [B, cap] view with row stride `stride` into a buffer whose padding holds a token that would match everything."""
    B, cap = hist.shape
    buf = torch.full((B, stride), 1, dtype=torch.int32, device="cuda:0")
    buf[:, :cap] = dev(hist)
    return buf[:, :cap]


def _check(hist, lengths, par, max_ngram, min_match, pad, stride):
    from qserve_amd import drafting as D
    h = _padded(hist, stride)
    out = torch.full((len(lengths), len(par)), -77, dtype=torch.int64, device=h.device)
    got = D.ngram_draft_tree(h, dev(np.asarray(lengths, np.int32)), dev(np.asarray(par, np.int64).astype(np.int32)), max_ngram, min_match,
                             pad, out=out)
    torch.cuda.synchronize()
    want = reference_draft_batch(hist, lengths, par, max_ngram, min_match, pad)
    assert got is out and torch.equal(got.cpu(), torch.from_numpy(want)), f"draft differs:\n{got.cpu().numpy()}\nexpected\n{want}"
    return want


@pytest.fixture(scope="module")
def histories():
    """One vocabulary-5 history per batch of LENGTHS (every column filled: what lies behind a length must not matter)."""
    rng = np.random.default_rng(21)
    return [rng.integers(0, 5, size=(3, CAP)).astype(np.int32) for _ in LENGTHS]


@pytest.mark.parametrize("ngram", NGRAMS, ids=lambda x: f"ngram{x[0]}-min{x[1]}")
@pytest.mark.parametrize("tree", list(TREES))
def test_draft_on_a_vocabulary_of_five(gpu, histories, tree, ngram):
    par = TREES[tree]
    drafted = 0
    for hist, lengths in zip(histories, LENGTHS):
        for pad in (-1, 0):                              # a pad outside the vocabulary, and one that is a token of it
            want = _check(hist, lengths, par, ngram[0], ngram[1], pad, STRIDE)
            drafted += int((want[:, 1:] != pad).sum())
    assert len(par) == 1 or drafted > 0, "every node was pad: nothing but the empty result was compared"


def test_draft_without_repeats_is_the_root_and_pad(gpu):
    """A vocabulary of 50 000 and no token twice: no context occurs earlier, every node but the root is pad."""
    rng = np.random.default_rng(22)
    hist = rng.permutation(50000)[:3 * CAP].reshape(3, CAP).astype(np.int32)
    for lengths in LENGTHS:
        want = _check(hist, lengths, TREES["par12"], 16, 1, -1, STRIDE)
        assert (want[:, 1:] == -1).all()


def test_draft_on_both_sides_of_the_lds_capacity(gpu):
    """One sequence each at LDS_TOKENS - 1, LDS_TOKENS (staged in LDS) and LDS_TOKENS + 1 (read from global memory): the same rule
    on both paths and at the seam."""
    from qserve_amd import drafting as D
    T = D.LDS_TOKENS
    rng = np.random.default_rng(23)
    hist = rng.integers(0, 5, size=(3, T + 1)).astype(np.int32)
    lengths = [T - 1, T, T + 1]
    for tree, ngram in (("par12", (16, 1)), ("tree64", (3, 2))):
        want = _check(hist, lengths, TREES[tree], ngram[0], ngram[1], -1, T + 1)       # (hist_stride == cap here)
        assert (want[:, 1:] != -1).any()
    # the global-memory path alone, on a history whose best matches lie behind the LDS capacity: a chain planted at the very end
    hist2 = rng.integers(0, 50000, size=(1, T + 1)).astype(np.int32)
    hist2[0, T - 5:T + 1] = [7, 8, 9, 10, 7, 8]
    want = _check(hist2, [T + 1], TREES["chain5"], 4, 2, -1, T + 1)
    assert want[0].tolist() == [8, 9, 10, 7, 8]


def test_draft_on_malformed_parents(gpu):
    """The values the header defines for a parent entry outside 0 .. i - 1: pad for the node, the rule for its descendants.  (No address
    is formed from such an entry.)"""
    rng = np.random.default_rng(24)
    hist = rng.integers(0, 5, size=(3, CAP)).astype(np.int32)
    for pad in (2, -1):
        want = _check(hist, LENGTHS[0], MALFORMED, 4, 1, pad, STRIDE)
        assert all((want[:, i] == pad).all() for i, a in enumerate(MALFORMED) if i and not 0 <= a < i)
        if pad == 2:
            assert (want[1:, 7] != pad).any()             # node 7, a child of the malformed node 6, continued "... 2" from the history


def test_draft_allocates_its_output_and_takes_an_empty_batch(gpu):
    from qserve_amd import drafting as D
    hist = np.array([[3, 4, 3, 4, 3]], np.int32)
    got = D.ngram_draft_tree(dev(hist), dev(np.array([5], np.int32)), dev(np.array([-1, 0, 1], np.int32)))
    assert got.dtype == torch.int64 and got.tolist() == [[3, 4, 3]]
    empty = D.ngram_draft_tree(torch.zeros((0, 8), dtype=torch.int32, device=gpu), torch.zeros((0,), dtype=torch.int32, device=gpu),
                               dev(np.array([-1, 0], np.int32)))
    assert tuple(empty.shape) == (0, 2)
    with pytest.raises(RuntimeError, match="max_ngram"):
        D.ngram_draft_tree(dev(hist), dev(np.array([5], np.int32)), dev(np.array([-1, 0], np.int32)), max_ngram=17)


# ---- the append ------------------------------------------------------------------------------------------------------------------
def test_history_append_is_the_numpy_statement(gpu):
    """B = 5, n = 6, cap = 20 in rows of stride 24: the bonus token alone (m = 1), the whole tree (m = n), ragged m, a row clipped at cap
    in the middle of its path, a row that begins beyond cap; every other element of the buffer - padding included - unchanged."""
    from qserve_amd import drafting as D
    rng = np.random.default_rng(25)
    B, n, cap, stride = 5, 6, 20, 24
    buf0 = rng.integers(1000, 2000, size=(B, stride)).astype(np.int32)
    past = np.array([4, 2, 9, 17, 25], np.int32)
    lens = np.array([1, n, 3, 5, 2], np.int32)
    idx = np.zeros((B, n), np.int32)
    for b in range(B):
        idx[b, 1:lens[b]] = np.sort(rng.permutation(np.arange(1, n))[:lens[b] - 1])
    nodes = rng.integers(0, 500, size=(B, n)).astype(np.int64)
    nxt = rng.integers(500, 900, size=(B,)).astype(np.int64)
    buf = dev(buf0)
    ret = D.history_append(buf[:, :cap], dev(past), dev(nodes), dev(idx), dev(lens), dev(nxt))
    torch.cuda.synchronize()
    want = buf0.copy()
    want[:, :cap] = reference_append(buf0[:, :cap], past, nodes, idx, lens, nxt)
    assert ret.data_ptr() == buf.data_ptr()
    assert torch.equal(buf.cpu(), torch.from_numpy(want)), "history differs from the numpy statement"
    # what the cases are there for: rows 0 - 2 written in full, row 3 clipped after cap - 1 - 17 = 2 tokens, row 4 untouched
    changed = (want != buf0).sum(axis=1).tolist()
    assert changed == [1, n, 3, 2, 0], changed
    # max_accept below n: accept_idx [B, 3], accept_lens cut to it
    buf = dev(buf0)
    D.history_append(buf[:, :cap], dev(past), dev(nodes), dev(np.ascontiguousarray(idx[:, :3])), dev(np.minimum(lens, 3)), dev(nxt))
    want = buf0.copy()
    want[:, :cap] = reference_append(buf0[:, :cap], past, nodes, idx[:, :3], np.minimum(lens, 3), nxt)
    assert torch.equal(buf.cpu(), torch.from_numpy(want))
