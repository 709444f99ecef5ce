"""`qs_logprob_rows` on the GPU against the float64 oracle of tests/_logprob_cases.py: log-probabilities within TOL(lp) = 1e-5 +
2^-21 * |lp| (derived next to the constant), ranks and top-list ids exactly.

Every logits buffer has its padding behind n filled with +65504 canaries, which must never be listed, ranked or summed; every output has
guard entries behind it (and, in the path form, sentinel columns around the written ones) which must stay untouched."""
import numpy as np
import pytest
import torch

from _logprob_cases import assert_close, expected_logs, score, slots

pytestmark = pytest.mark.gpu

SHAPES = [(1, 8, 8), (3, 1000, 1008), (2, 1003, 1008), (2, 128256, 128256), (64, 4096, 4104)]
TINY8, SMALL, ODD, BIG, WIDE = SHAPES
CANARY = 65504.0
NEG = -np.inf


def _device_rows(gpu, x, stride):
    rows, n = x.shape
    buf = torch.full((rows, stride), CANARY, dtype=torch.float16, device=gpu)
    buf[:, :n] = torch.from_numpy(x).to(gpu)
    return buf[:, :n]


def _random(shape, seed, sigma=3.0):
    rows, n, _ = shape
    return (np.random.default_rng(seed).standard_normal((rows, n)) * sigma).astype(np.float16)


def _run(gpu, x, ids, stride, T=1.0, top=0):
    """The plain form on numpy rows, into outputs with two guard rows -> (lp, rank, top_ids, top_lp) numpy (the lists [rows, top])."""
    from qserve_amd.logprobs import logprob_rows
    rows = x.shape[0]
    lp = torch.full((rows + 2,), -7.0, dtype=torch.float32, device=gpu)
    rank = torch.full((rows + 2,), -7, dtype=torch.int32, device=gpu)
    tids = torch.full((rows + 2, top), -7, dtype=torch.int32, device=gpu)
    tlp = torch.full((rows + 2, top), -7.0, dtype=torch.float32, device=gpu)
    if isinstance(T, np.ndarray):
        T = torch.from_numpy(T.astype(np.float32)).to(gpu)
    res = logprob_rows(_device_rows(gpu, x, stride), torch.from_numpy(np.asarray(ids, dtype=np.int64)).to(gpu), T, top,
                       out=(lp[:rows], rank[:rows], tids[:rows], tlp[:rows]))
    torch.cuda.synchronize()
    assert (res[2] is None) == (top == 0)
    for t in (lp, rank, tids, tlp):
        assert (t[rows:].cpu().numpy() == -7).all(), "an output was written behind `rows`"
    return lp[:rows].cpu().numpy(), rank[:rows].cpu().numpy(), tids[:rows].cpu().numpy(), tlp[:rows].cpu().numpy()


def _check(gpu, x, ids, stride, T=1.0, top=0, what=""):
    """Run and compare every row with the oracle -> the kernel's outputs."""
    lp, rank, tids, tlp = _run(gpu, x, ids, stride, T, top)
    Ts = np.broadcast_to(np.asarray(T, dtype=np.float32), (x.shape[0],))
    want = [score(x[r], int(ids[r]), Ts[r], top) for r in range(x.shape[0])]
    assert rank.tolist() == [w[1] for w in want], f"{what}: ranks differ"
    assert tids.tolist() == [w[2] for w in want], f"{what}: top ids differ"
    assert_close(lp, [w[0] for w in want], f"{what} lp")
    assert_close(tlp, np.array([w[3] for w in want]).reshape(x.shape[0], top), f"{what} top lp")
    return lp, rank, tids, tlp


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("T", [1.0, 0.7, 2.0])
def test_random_rows_against_the_oracle(gpu, shape, T):
    rows, n, stride = shape
    x = _random(shape, 300 + n)
    rng = np.random.default_rng(n)
    for top in (0, 1, 5, 32):
        ids = rng.integers(0, n, size=rows)
        ids[0] = int(np.argmax(x[0].astype(np.float32)))                     # one row scores its maximum
        _check(gpu, x, ids, stride, T, top, f"{shape} T={T} top={top}")


def test_a_list_longer_than_the_row(gpu):
    """top = 32 at n = 8: eight entries, then id -1 / lp -inf."""
    x = _random(TINY8, 5)
    _, _, tids, tlp = _check(gpu, x, [3], 8, 1.0, 32, "top=32 at n=8")
    assert sorted(tids[0, :8].tolist()) == list(range(8)) and tids[0, 8:].tolist() == [-1] * 24 and np.isneginf(tlp[0, 8:]).all()


def test_an_all_equal_row_of_128256_logits(gpu):
    rows, n, stride = BIG
    x = np.full((rows, n), 1.5, dtype=np.float16)
    for top, ids in ((5, [17, n - 1]), (32, [0, 64000])):
        lp, rank, tids, tlp = _check(gpu, x, ids, stride, 0.7, top, f"all-equal top={top}")
        assert rank.tolist() == [t + 1 for t in ids] and tids.tolist() == [list(range(top))] * rows
        assert np.abs(lp + np.log(n)).max() < 2e-5


def test_a_tie_class_at_the_threshold_larger_than_what_is_left(gpu):
    """Three values above, then a class of 300 equal values spread over the row (and over the 1024-unit chunks of the selection): the
    list takes the three, then the first top - 3 ids of the class in index order."""
    for shape in (SMALL, ODD, BIG):
        rows, n, stride = shape
        rng = np.random.default_rng(n)
        x = (rng.standard_normal((rows, n)) * 0.5 - 4.0).astype(np.float16)
        tie = np.sort(rng.choice(n, size=300, replace=False))
        above = rng.choice(np.setdiff1d(np.arange(n), tie), size=3, replace=False)
        x[:, tie] = 2.0
        x[:, above] = np.array([5.0, 3.0, 4.0], dtype=np.float16)
        for top in (5, 20, 32):
            _, rank, tids, _ = _check(gpu, x, [int(tie[150]), int(tie[0])][:rows] + [int(above[1])] * (rows - 2), stride, 1.0, top,
                                      f"tie class {shape} top={top}")
            assert tids[0].tolist() == [int(above[0]), int(above[2]), int(above[1])] + tie[:top - 3].tolist()
            assert rank[0] == 3 + 150 + 1


def test_a_repeated_maximum_and_a_dominant_logit(gpu):
    rows, n, stride = SMALL
    x = _random(SMALL, 9)
    x[:, [7, 500, 999]] = 30.0                                              # the maximum three times: ranks 1, 2, 3 by index
    _, rank, tids, _ = _check(gpu, x, [500, 999, 7], stride, 1.0, 5, "repeated maximum")
    assert rank.tolist() == [2, 3, 1] and tids[:, :3].tolist() == [[7, 500, 999]] * 3
    x = (_random(SMALL, 10, 1.0) - 20.0).astype(np.float16)
    x[:, 123] = 40.0                                                        # 60 above the rest: lp ~ 0 for it, ~ -60 for the others
    lp, _, _, _ = _check(gpu, x, [123, 124, 0], stride, 1.0, 5, "dominant logit")
    assert abs(lp[0]) < 1e-5 and lp[1] < -50


def test_extreme_temperatures(gpu):
    rows, n, stride = ODD
    x = _random(ODD, 11)
    ids = [5, n - 1]
    _check(gpu, x, ids, stride, 100.0, 5, "T=100")
    _check(gpu, x, ids, stride, 1e-3, 5, "T=1e-3")
    greedy = _check(gpu, x, ids, stride, 1e-6, 5, "T=1e-6 (greedy: reported at T = 1)")
    plain = _run(gpu, x, ids, stride, 1.0, 5)
    for a, b in zip(greedy, plain):
        assert np.array_equal(a, b, equal_nan=True)


def test_masked_rows(gpu):
    """-inf logits: never listed, weigh nothing; fewer finite logits than `top`; a chosen id that is masked."""
    rows, n, stride = SMALL
    x = _random(SMALL, 12)
    x[0, ::2] = NEG
    x[1, :] = NEG
    keep = [3, 400, 998]
    x[1, keep] = np.array([1.0, 2.0, 1.0], dtype=np.float16)               # three finite logits
    x[2, 100:900] = NEG
    lp, rank, tids, tlp = _check(gpu, x, [4, 5, 500], stride, 0.7, 5, "masked")
    assert np.isneginf(lp).all()                                             # all three chosen ids are masked
    assert tids[1].tolist() == [400, 3, 998, -1, -1] and np.isneginf(tlp[1, 3:]).all()
    assert rank[1] == 3 + 4 + 1                                              # behind the three finite ones and the masked ids 0, 1, 2, 4
    _check(gpu, x, [1, 400, 50], stride, 1.0, 32, "masked, finite ids")


def test_the_last_id_of_an_odd_row_and_ids_out_of_range(gpu):
    rows, n, stride = ODD
    x = _random(ODD, 13)
    x[0, n - 1] = x[0].max() + np.float16(1.0)                               # the last element, next to the canaries, is the maximum
    _, rank, tids, _ = _check(gpu, x, [n - 1, n - 1], stride, 1.0, 5, "id n - 1")
    assert rank[0] == 1 and tids[0, 0] == n - 1
    for bad in ([n, -1], [1 << 40, -(1 << 40)], [n + 4, 1 << 31]):           # (n + 4: inside the padding of the row)
        lp, rank, tids, tlp = _check(gpu, x, bad, stride, 1.0, 5, f"ids {bad}")
        assert np.isnan(lp).all() and rank.tolist() == [0, 0] and (tids >= 0).all()


def test_per_sequence_temperatures(gpu):
    rows, n, stride = WIDE
    x = _random(WIDE, 14)
    rng = np.random.default_rng(15)
    T = rng.choice(np.array([0.5, 0.7, 1.0, 2.0, 1e-6], dtype=np.float32), size=rows)
    _check(gpu, x, rng.integers(0, n, size=rows), stride, T, 5, "per-sequence T")


PAR_N = 12


def _path_case(lens, lengths, seed):
    """B = 3, a 12-node tree: random drafts, paths that are random node sequences (the kernel takes the walk's word for them), one entry
    out of range."""
    rng = np.random.default_rng(seed)
    B, n, V = 3, PAR_N, 1000
    x = (rng.standard_normal((B * n, V)) * 3.0).astype(np.float16)
    node_tokens = rng.integers(0, V, size=(B, n))
    accept_idx = np.stack([np.concatenate(([0], 1 + rng.permutation(n - 1))) for _ in range(B)]).astype(np.int32)
    accept_idx[2, 3] = 40                                                    # clamped to node 11
    return dict(x=x, node_tokens=node_tokens, accept_idx=accept_idx, accept_lens=np.asarray(lens, dtype=np.int32),
                next_token=rng.integers(0, V, size=B), lengths=None if lengths is None else np.asarray(lengths, dtype=np.int32))


def _run_path(gpu, c, top, cols, T=1.0, rank=True):
    from qserve_amd.logprobs import logprob_path
    B, n = c["node_tokens"].shape
    dev = lambda a, dt: None if a is None else torch.from_numpy(np.asarray(a).astype(dt)).to(gpu)   # noqa: E731
    wide = cols + 3                                                          # the logs are views of wider buffers: guard columns
    out = (torch.full((B + 1, wide), -7.0, dtype=torch.float32, device=gpu), torch.full((B + 1, wide), -7, dtype=torch.int32, device=gpu),
           torch.full((B + 1, wide, top), -7, dtype=torch.int32, device=gpu), torch.full((B + 1, wide, top), -7.0, dtype=torch.float32, device=gpu))
    view = tuple(t[:B, :cols] for t in out)
    if not rank:
        view = (view[0], None, view[2], view[3])
    if isinstance(T, np.ndarray):
        T = torch.from_numpy(T.astype(np.float32)).to(gpu)
    logprob_path(_device_rows(gpu, c["x"], 1008), dev(c["node_tokens"], np.int64), dev(c["accept_idx"], np.int32), dev(c["accept_lens"], np.int32),
                 dev(c["next_token"], np.int64), dev(c["lengths"], np.int32), T, top, out=view)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


@pytest.mark.parametrize("lens,lengths", [((0, 1, 5), (20, 0, 33)), ((12, 5, 1), (3, 30, 36)), ((12, 0, 5), None), ((20, -3, 12), (0, 9, 33))],
                         ids=str)
def test_the_path_form(gpu, lens, lengths):
    """Path lengths 0, 1, 5 and 12 (and counts outside 0 .. max_accept): dead slots untouched, columns by `lengths` (36 columns: every
    case with `lengths` has a path that runs beyond them and is cut there), or j - 1 without `lengths`."""
    c = _path_case(lens, lengths, 20 + sum(abs(v) for v in lens))
    B, n, cols, top = 3, PAR_N, 36, 5
    T = np.array([1.0, 0.7, 2.0], dtype=np.float32)
    written = slots(c["node_tokens"], c["accept_idx"], c["accept_lens"], c["next_token"], c["lengths"], B, n, n, cols)
    m = np.clip(c["accept_lens"], 0, n)
    assert len(written) == int(m.sum()) if lengths is None else 0 < len(written) < int(m.sum()), "with `lengths` the case must cut a column"
    want = expected_logs(c["x"], written, T, top, B, cols)
    got = _run_path(gpu, c, top, cols, T)
    hit = np.zeros((B, cols), dtype=bool)
    for b, _, _, _, col in written:
        hit[b, col] = True
    for g in got:                                                            # guard row, guard columns and every column no slot owns
        assert (g[B:] == -7).all() and (g[:B, cols:] == -7).all() and (g[:B, :cols][~hit] == -7).all(), "a dead slot or a guard was written"
    assert np.array_equal(got[1][:B, :cols][hit], want[1][hit]), "ranks differ"
    assert np.array_equal(got[2][:B, :cols][hit], want[2][hit]), "top ids differ"
    assert_close(got[0][:B, :cols][hit], want[0][hit], f"path {lens} lp")
    assert_close(got[3][:B, :cols][hit], want[3][hit], f"path {lens} top lp")
    # the same call without a rank output: everything else bit-equal, the rank buffer untouched
    again = _run_path(gpu, c, top, cols, T, rank=False)
    assert (again[1] == -7).all()
    for i in (0, 2, 3):
        assert np.array_equal(again[i], got[i], equal_nan=True)


def test_a_step_with_a_count_per_sequence(gpu):
    """The form a decode step with stopping uses: n = 1, no draft, accept_lens = the stop rule's k (0 / 1), columns by `lengths`."""
    from qserve_amd.logprobs import logprob_path, new_logs
    B, V = 3, 1000
    x = _random((B, V, 1008), 31)
    nxt, lengths, k = np.array([5, 999, 17]), np.array([4, 7, 2], dtype=np.int32), np.array([1, 0, 1], dtype=np.int32)
    out = new_logs(B, 8, 3, gpu)
    logprob_path(_device_rows(gpu, x, 1008), None, None, torch.from_numpy(k).to(gpu), torch.from_numpy(nxt).to(gpu),
                 torch.from_numpy(lengths).to(gpu), 1.0, 3, out=out)
    torch.cuda.synchronize()
    written = slots(None, None, k, nxt, lengths, B, 1, 1, 8)
    assert [(s[0], s[4]) for s in written] == [(0, 4), (2, 2)]
    want = expected_logs(x, written, 1.0, 3, B, 8)
    got = [t.cpu().numpy() for t in out]
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert_close(got[0], want[0], "step lp")
    assert_close(got[3], want[3], "step top lp")


@pytest.mark.parametrize("shape", [SMALL, BIG], ids=str)
def test_deterministic_and_capturable(gpu, shape):
    """The same call twice: bit-equal.  Captured and replayed twice: bit-equal to eager."""
    from qserve_amd.logprobs import logprob_rows, new_logs
    rows, n, stride = shape
    x = _random(shape, 40)
    x[0, ::3] = x[0, 1]                                                      # a large tie class in one row
    xd = _device_rows(gpu, x, stride)
    ids = torch.from_numpy(np.random.default_rng(41).integers(0, n, size=rows)).to(gpu)
    T = torch.full((rows,), 0.7, dtype=torch.float32, device=gpu)

    def fresh():
        return tuple(t.squeeze(1) for t in new_logs(rows, 1, 20, gpu))

    a, b, c = fresh(), fresh(), fresh()
    logprob_rows(xd, ids, T, 20, out=a)
    logprob_rows(xd, ids, T, 20, out=b)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        logprob_rows(xd, ids, T, 20, out=c)
    for i in range(2):
        for t in c:
            t.fill_(-3)
        g.replay()
        torch.cuda.synchronize()
        for name, ta, tb, tc in zip(("lp", "rank", "top_ids", "top_lp"), a, b, c):
            bits = lambda t: t.view(torch.int32)                             # noqa: E731
            assert torch.equal(bits(ta), bits(tb)), f"{name}: two eager calls differ"
            assert torch.equal(bits(ta), bits(tc)), f"{name}: replay {i} differs from eager"
    assert not torch.isnan(a[0]).any() and int(a[1].min()) >= 1
