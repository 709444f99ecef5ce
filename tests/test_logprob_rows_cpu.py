"""`qs_logprob_rows` without a GPU: the argument validation of the built library (which happens before any HIP call, on made-up
addresses), the rejections of the `qserve_amd.logprobs` wrappers, and self-checks of the float64 oracle of tests/_logprob_cases.py - an
all-equal row, masked logits, and the slot rule on a hand-written path."""
import numpy as np
import pytest
import torch

from _logprob_cases import TOL, keys, log_softmax, score, slots


def test_argument_validation_without_gpu(built_lib):
    from qserve_amd._lib import lib

    def call(logits=4096, stride=16, V=16, node_tokens=None, accept_idx=None, accept_lens=None, next_token=8192, lengths=None, batch=2, n=1,
             max_accept=1, seq_t=None, top=0, out_lp=12288, out_rank=16384, top_ids=None, top_lp=None, out_stride=4, out_cols=4):
        return lib.qs_logprob_rows(logits, stride, V, node_tokens, accept_idx, accept_lens, next_token, lengths, batch, n, max_accept, 1.0,
                                   seq_t, top, out_lp, out_rank, top_ids, top_lp, out_stride, out_cols, None)

    assert call(logits=None) == -1 and b"null pointer" in lib.qs_last_error()
    assert call(next_token=None) == -1 and call(out_lp=None) == -1
    assert call(V=7, stride=8) == -1 and b"n_vocab=7" in lib.qs_last_error()
    assert call(V=(1 << 22) + 8, stride=(1 << 22) + 8) == -1
    assert call(V=16, stride=20) == -1                                       # a stride that is no multiple of 8
    assert call(V=24, stride=16) == -1                                       # a stride below n_vocab
    assert call(logits=4104) == -1 and b"16-byte" in lib.qs_last_error()
    assert call(next_token=8196) == -1 and b"8-byte" in lib.qs_last_error()
    assert call(node_tokens=20484, accept_idx=24576, accept_lens=28672, n=4, max_accept=4) == -1 and b"8-byte" in lib.qs_last_error()
    for name in ("accept_lens", "lengths", "seq_t", "out_lp", "out_rank"):
        assert call(**{name: 32770}) == -1 and b"4-byte" in lib.qs_last_error(), name
    assert call(top=5, top_ids=36864, top_lp=40962) == -1 and b"4-byte" in lib.qs_last_error()
    for n in (0, 65):
        assert call(n=n, node_tokens=20480) == -1 and f"n={n}".encode() in lib.qs_last_error()
        assert call(max_accept=n, accept_idx=24576) == -1 and f"max_accept={n}".encode() in lib.qs_last_error()
    for top in (-1, 33):
        assert call(top=top, top_ids=36864, top_lp=40960) == -1 and f"top={top}".encode() in lib.qs_last_error()
    assert call(top=5) == -1 and call(top=5, top_ids=36864) == -1 and call(top=5, top_lp=40960) == -1
    assert b"top=5 needs" in lib.qs_last_error()
    assert call(n=2) == -1 and b"node_tokens is null" in lib.qs_last_error()
    assert call(max_accept=2) == -1 and b"accept_idx is null" in lib.qs_last_error()
    assert call(out_stride=3, out_cols=4) == -1 and b"out_stride=3" in lib.qs_last_error()
    assert call(batch=-1) == -1 and call(batch=65536) == -1 and b"batch=65536" in lib.qs_last_error()
    assert call(batch=0) == 0                                                # nothing to do: no launch
    assert call(batch=0, top=32, top_ids=36864, top_lp=40960, n=64, max_accept=64, node_tokens=20480, accept_idx=24576) == 0


def test_wrapper_rejections(built_lib):
    from qserve_amd.logprobs import MAX_TOP, logprob_path, logprob_rows
    assert MAX_TOP == 32
    x, ids = torch.zeros((3, 16), dtype=torch.float16), torch.zeros((3,), dtype=torch.int64)
    with pytest.raises(RuntimeError, match="scalar type"):
        logprob_rows(x.float(), ids)
    with pytest.raises(RuntimeError, match=r"logits must be \[rows, n\]"):
        logprob_rows(x[0], ids)
    with pytest.raises(RuntimeError, match=r"logits must be \[rows, n\]"):
        logprob_rows(x.t(), ids)
    with pytest.raises(RuntimeError, match="n=7"):
        logprob_rows(torch.zeros((3, 8), dtype=torch.float16)[:, :7], ids)
    with pytest.raises(RuntimeError, match="row stride 12"):
        logprob_rows(torch.zeros((3, 12), dtype=torch.float16)[:, :8], ids)
    with pytest.raises(RuntimeError, match="top=33"):
        logprob_rows(x, ids, top=33)
    with pytest.raises(RuntimeError, match="ids must be"):
        logprob_rows(x, ids[:2])
    with pytest.raises(RuntimeError, match="scalar type"):
        logprob_rows(x, ids.int())
    with pytest.raises(RuntimeError, match="temperature must be"):
        logprob_rows(x, ids, temperature=torch.ones((2,)))
    with pytest.raises(RuntimeError, match="CUDA"):                          # everything right but the device
        logprob_rows(x, ids)
    tree = dict(node_tokens=torch.zeros((3, 4), dtype=torch.int64), accept_idx=torch.zeros((3, 4), dtype=torch.int32),
                accept_lens=torch.ones((3,), dtype=torch.int32), next_token=ids)
    x4 = torch.zeros((12, 16), dtype=torch.float16)
    with pytest.raises(RuntimeError, match="come together"):
        logprob_path(x4, **dict(tree, accept_idx=None))
    with pytest.raises(RuntimeError, match="needs its accept_lens"):
        logprob_path(x4, **dict(tree, accept_lens=None))
    with pytest.raises(RuntimeError, match="logits has 3 rows"):
        logprob_path(x, **tree)
    with pytest.raises(RuntimeError, match="node_tokens must be"):
        logprob_path(x4, **dict(tree, node_tokens=torch.zeros((3, 65), dtype=torch.int64)))
    with pytest.raises(RuntimeError, match="lengths must be"):
        logprob_path(x4, lengths=torch.zeros((2,), dtype=torch.int32), **tree)
    with pytest.raises(RuntimeError, match="scalar type"):
        logprob_path(x4, **dict(tree, next_token=ids.int()))
    outs = (torch.zeros((3, 6)), torch.zeros((3, 6), dtype=torch.int32), torch.zeros((3, 6, 2), dtype=torch.int32), torch.zeros((3, 6, 2)))
    with pytest.raises(RuntimeError, match="out rank must be"):
        logprob_path(x4, top=2, out=(outs[0], outs[1][:, :5], outs[2], outs[3]), **tree)
    with pytest.raises(RuntimeError, match="out top_ids must be"):
        logprob_path(x4, top=2, out=(outs[0], outs[1], torch.zeros((3, 6, 3), dtype=torch.int32), outs[3]), **tree)
    with pytest.raises(RuntimeError, match="out top_lp must be"):           # another row stride than lp's
        logprob_path(x4, top=2, out=(outs[0], outs[1], outs[2], torch.zeros((3, 8, 2))[:, :6]), **tree)
    with pytest.raises(RuntimeError, match="both top lists"):
        logprob_path(x4, top=2, out=(outs[0], outs[1], None, outs[3]), **tree)
    with pytest.raises(RuntimeError, match="CUDA"):
        logprob_path(x4, top=2, out=outs, **tree)


def test_the_key_orders_like_the_value():
    v = np.array([-np.inf, -65504, -1, -6e-8, -0.0, 0.0, 6e-8, 1, 65504, np.inf], dtype=np.float16)
    k = keys(v)
    assert k[4] == k[5] and k[0] == 0x03FF
    assert (np.diff(np.delete(k, 4)) > 0).all()


def test_oracle_on_an_all_equal_row():
    n = 128256
    x = np.full(n, 1.5, dtype=np.float16)
    for t in (0, 17, n - 1):
        lp, rank, ids, lps = score(x, t, 0.7, 5)
        assert abs(lp + np.log(n)) < 1e-12 and rank == t + 1 and ids == [0, 1, 2, 3, 4] and all(abs(v + np.log(n)) < 1e-12 for v in lps)
    assert TOL(-np.log(n)) < 2e-5


def test_oracle_masks_and_ties_and_range():
    x = np.array([1, 3, 3, -np.inf, 2, 3, 0, -np.inf], dtype=np.float16)
    lp, rank, ids, lps = score(x, 5, 1.0, 8)
    assert rank == 3 and ids == [1, 2, 5, 4, 0, 6, -1, -1] and lps[6:] == [-np.inf, -np.inf]
    assert abs(sum(np.exp(lps[:6])) - 1.0) < 1e-12 and lp == lps[2]
    assert score(x, 3, 1.0, 0)[:2] == (-np.inf, 7) and score(x, 7, 1.0, 0)[1] == 8         # masked ids rank behind everything, by index
    for t in (-1, 8, 1 << 40):
        lp, rank, ids, _ = score(x, t, 1.0, 2)
        assert np.isnan(lp) and rank == 0 and ids == [1, 2]
    assert np.array_equal(log_softmax(x, 1e-6), log_softmax(x, 1.0))          # a greedy temperature reports the untempered values
    assert abs(log_softmax(x, 2.0)[4] - (1.0 - np.log(3 * np.exp(1.5) + np.exp(1.0) + np.exp(0.5) + 1.0))) < 1e-12


def test_slot_rule_on_a_hand_written_path():
    """B = 2, a 5-node tree.  Sequence 0 accepted the path 0 -> 2 -> 4 (m = 3) at L = 10: node 2's token is scored on row 0 at column 10,
    node 4's on row 2 at column 11, the bonus token on row 4 at column 12.  Sequence 1 accepted nothing (m = 0)."""
    node_tokens = np.array([[50, 51, 52, 53, 54], [60, 61, 62, 63, 64]])
    accept_idx = np.array([[0, 2, 4, 0, 0], [0, 1, 0, 0, 0]])
    kw = dict(node_tokens=node_tokens, accept_idx=accept_idx, next_token=np.array([99, 98]), batch=2, n=5, max_accept=5)
    got = slots(accept_lens=np.array([3, 0]), lengths=np.array([10, 20]), out_cols=32, **kw)
    assert got == [(0, 1, 0, 52, 10), (0, 2, 2, 54, 11), (0, 3, 4, 99, 12)]
    # clipped to k = 2 by the stop rule, which also rewrote next_token to e_2 = node 4's token: the same arrays describe the clipped path
    kw2 = dict(kw, next_token=np.array([54, 98]))
    assert slots(accept_lens=np.array([2, 0]), lengths=np.array([10, 20]), out_cols=32, **kw2) == got[:1] + [(0, 2, 2, 54, 11)]
    # without lengths the columns are j - 1; columns beyond out_cols are skipped; m is cut to max_accept; indices are clamped
    assert [s[4] for s in slots(accept_lens=np.array([3, 1]), lengths=None, out_cols=2, **kw)] == [0, 1, 0]
    assert len(slots(accept_lens=np.array([9, 0]), lengths=None, out_cols=32, **kw)) == 5
    wild = dict(kw, accept_idx=np.array([[0, 7, -3, 0, 0], [0, 0, 0, 0, 0]]))
    assert slots(accept_lens=np.array([3, 0]), lengths=None, out_cols=32, **wild) == [(0, 1, 0, 54, 0), (0, 2, 4, 50, 1), (0, 3, 0, 99, 2)]
    # a plain batch of rows: one slot per row, scored for next_token
    plain = slots(None, None, None, np.array([7, 8]), None, 2, 1, 1, 1)
    assert plain == [(0, 1, 0, 7, 0), (1, 1, 1, 8, 0)]
    assert slots(None, None, np.array([0, 5]), np.array([7, 8]), np.array([3, 4]), 2, 1, 1, 8) == [(1, 1, 1, 8, 4)]
