"""`qs_beam_select` and `qs_rows_move` on the GPU, every named case of tests/_beam_cases.py: the candidate lists against the float64
oracle (ids exactly, lp within qs_logprob_rows' bound 1e-5 + 2^-21 |lp|) and bit for bit against `qs_logprob_rows(top = W)` on the same
rows; parent / next_token / cum_out / moved / src_rows bit for bit against the loop restatement of launch 2 fed with the device's own
candidate lists; on the gapped cases the chosen (parent, token) set against the float64 oracle alone; graph replay against the eager
run; the row move against its restatement.

Every logits buffer has its padding behind n filled with +65504 canaries; every output has guard rows behind it."""
import numpy as np
import pytest
import torch

import _beam_cases as K
from _logprob_cases import assert_close

pytestmark = pytest.mark.gpu

CASES = K.named_cases()
CANARY = 65504.0
NAMES = ("parent", "next_token", "cum_out", "moved", "src_rows")


def _padded(gpu, x):
    """The rows on the device at a row stride that is a multiple of 8, the padding behind n filled with canaries."""
    B, n = x.shape
    buf = torch.full((B, (n + 7) // 8 * 8 + 8), CANARY, dtype=torch.float16, device=gpu)
    buf[:, :n] = torch.from_numpy(x).to(gpu)
    return buf[:, :n]


def _inputs(gpu, case):
    return _padded(gpu, case["logits"]), *(torch.from_numpy(case[k]).to(gpu) for k in ("cum", "finished", "tokens"))


def _outputs(gpu, B, W):
    """Outputs with two guard rows, filled with -7."""
    spec = ((torch.int32, ()), (torch.int64, ()), (torch.float32, ()), (torch.int32, ()), (torch.int32, ()), (torch.int32, (W,)),
            (torch.float32, (W,)))
    return [torch.full((B + 2, *tail), -7, dtype=dt, device=gpu) for dt, tail in spec]


def _select(gpu, case, inputs=None):
    """-> the seven outputs as numpy arrays, after checking the guard rows."""
    from qserve_amd import beams
    B, W = case["cum"].size, case["W"]
    full = _outputs(gpu, B, W)
    beams.select(*(inputs or _inputs(gpu, case)), W, out=tuple(t[:B] for t in full))
    torch.cuda.synchronize()
    for t in full:
        assert (t[B:].cpu().numpy() == -7).all(), "an output was written behind the batch"
    return [t[:B].cpu().numpy() for t in full]


@pytest.fixture(scope="module")
def results(gpu):
    """Every case once, shared by the tests below (read only)."""
    return {name: _select(gpu, case) for name, case in CASES.items()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_candidates_against_the_oracle_and_against_logprob_rows(gpu, results, name):
    from qserve_amd.logprobs import logprob_rows
    case = CASES[name]
    W = case["W"]
    ids, lp = results[name][5:]
    want_ids, want_lp = K.candidates_oracle(case["logits"], case["cum"], case["finished"], W)
    assert np.array_equal(ids, want_ids), f"{name}: candidate ids differ from the oracle's"
    assert_close(lp, want_lp, f"{name} candidate lp")
    live = np.nonzero((case["cum"] != K.NEG) & (case["finished"] == 0))[0]
    if live.size:
        rows = _padded(gpu, case["logits"][live])
        _, _, tids, tlp = logprob_rows(rows, torch.zeros((live.size,), dtype=torch.int64, device=gpu), 1.0, W)
        assert np.array_equal(tids.cpu().numpy(), ids[live])
        assert np.array_equal(tlp.cpu().numpy().view(np.uint32), lp[live].view(np.uint32)), f"{name}: lp bits differ from qs_logprob_rows'"


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_choice_is_bit_equal_to_the_restatement_on_the_device_lists(results, name):
    case = CASES[name]
    got = results[name]
    want = K.merge_loop(case["cum"], case["finished"], case["tokens"], got[5], got[6], case["W"])
    for key, g in zip(NAMES, got):
        w = want[key]
        assert g.dtype == w.dtype and np.array_equal(g.view(np.uint8), w.view(np.uint8)), f"{name}: {key} {g} != {w}"


@pytest.mark.parametrize("name", K.gap_cases(CASES))
def test_gapped_cases_choose_what_the_float64_oracle_chooses(results, name):
    case = CASES[name]
    W = case["W"]
    parent, nxt, out = results[name][:3]
    for g, cands in enumerate(K.exact_scores(case)):
        rows = range(g * W, g * W + W)
        got = sorted((int(parent[d]), int(nxt[d])) for d in rows if out[d] != K.NEG)
        assert got == sorted((b, t) for _, b, _, t in cands[:W]), f"{name}: group {g}"


@pytest.mark.parametrize("name", ["random_w4_g3_n1000", "fewer_than_w", "frozen_rows", "random_w32_g3_n9"])
def test_graph_replay_is_bit_identical_to_the_eager_run(gpu, results, name):
    from qserve_amd import beams
    case = CASES[name]
    B, W = case["cum"].size, case["W"]
    inputs = _inputs(gpu, case)
    full = _outputs(gpu, B, W)
    out = tuple(t[:B] for t in full)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        beams.select(*inputs, W, out=out)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        beams.select(*inputs, W, out=out)
    for t in full:
        t.fill_(-7)
    graph.replay()
    torch.cuda.synchronize()
    for key, t, eager in zip(NAMES + ("cand_ids", "cand_lp"), full, results[name]):
        assert np.array_equal(t[:B].cpu().numpy().view(np.uint8), eager.view(np.uint8)), f"{name}: {key} differs under replay"
        assert (t[B:].cpu().numpy() == -7).all()


# ---- the row move ---------------------------------------------------------------------------------------------------------------------
def _move(gpu, parent, tensors):
    from qserve_amd import beams
    dev = [torch.from_numpy(t.copy()).to(gpu) for t in tensors]
    err = torch.zeros((1,), dtype=torch.int32, device=gpu)
    beams.move_rows(torch.tensor(parent, dtype=torch.int32, device=gpu), dev, err)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in dev], int(err.cpu())


def _rows(B, row_bytes, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(B, row_bytes), dtype=np.uint8)


@pytest.mark.parametrize("parent", [[0, 0, 2, 2, 2, 5, 5], [0, 1, 2, 3, 4, 5, 6], [6, 6, 6, 6, 6, 6, 6]], ids=str)
def test_rows_of_4_20_and_4096_bytes_move_in_one_launch(gpu, parent):
    B = len(parent)
    tensors = [_rows(B, 4, 1).view(np.int32).reshape(B), _rows(B, 20, 2), _rows(B, 4096, 3).view(np.int32), _rows(B, 8, 4).view(np.int64)]
    got, err = _move(gpu, parent, tensors)
    want, want_err = K.move_loop(parent, tensors)
    assert err == want_err == 0
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


def test_a_misaligned_base_moves_by_bytes(gpu):
    from qserve_amd import beams
    B, parent = 5, [1, 1, 1, 3, 3]
    host = _rows(1, B * 48 + 16, 7).reshape(-1)
    buf = torch.from_numpy(host.copy()).to(gpu)
    view = buf[4:4 + B * 48].view(B, 48)                                    # rows of 48 bytes, a multiple of 16, at a base that is not
    assert view.data_ptr() % 16 == 4
    err = torch.zeros((1,), dtype=torch.int32, device=gpu)
    beams.move_rows(torch.tensor(parent, dtype=torch.int32, device=gpu), [view], err)
    torch.cuda.synchronize()
    want, _ = K.move_loop(parent, [host[4:4 + B * 48].reshape(B, 48)])
    after = buf.cpu().numpy()
    assert int(err.cpu()) == 0 and np.array_equal(after[4:4 + B * 48].reshape(B, 48), want[0])
    assert np.array_equal(after[:4], host[:4]) and np.array_equal(after[4 + B * 48:], host[4 + B * 48:])


def test_a_chain_sets_error_and_skips_the_row(gpu):
    tensors = [_rows(3, 4, 5).view(np.int32).reshape(3), _rows(3, 20, 6), _rows(3, 4096, 8)]
    got, err = _move(gpu, [1, 2, 2], tensors)
    want, want_err = K.move_loop([1, 2, 2], tensors)
    assert err == want_err == 1
    for g, w, t in zip(got, want, tensors):
        assert np.array_equal(g, w) and np.array_equal(g[0], t[0])           # row 0 <- row 1 <- row 2: row 0 is skipped
    got, err = _move(gpu, [7, 1, -3], tensors)                               # parents outside the batch
    assert err == 1 and all(np.array_equal(g, t) for g, t in zip(got, tensors))
