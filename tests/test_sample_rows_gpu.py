"""`qs_sample_rows` on the GPU against the float64 oracle of tests/_sample_cases.py.

A kernel token passes if, for some admissible survivor set (the exact one, and every value threshold whose tail mass is within DELTA * W
of p * W), it is in the set and CDF_lo(t) - DELTA <= u < CDF_hi(t) + DELTA, DELTA = 1e-4.  Planted cases keep a nucleus margin and a
distance of u from its token's CDF edges of at least 0.01 and must give the oracle's token exactly.  At least 90 % of the random cases
must have ONE admissible set (asserted on the oracle alone).

Every logits buffer has its padding behind n filled with +65504 canaries, which must never be returned, and `out` has two entries behind
`rows`, which must stay untouched.

Greedy equivalence: T = 1e-6 and p = 1e-9 are greedy by the contract and must equal qs_argmax_rows on rows with repeated maxima under
any u.  k = 1 is NOT a greedy condition of the contract: ties at the k-th value stay, so on a row with repeated maxima the draw goes over
all of them.  There k = 1 must equal qs_argmax_rows at u = 0 and on rows with one maximum under any u, and must return a maximum always."""
import numpy as np
import pytest
import torch

from _sample_cases import DELTA, U_MAX, Row, check_tokens, philox_uniform, position_keys

pytestmark = pytest.mark.gpu

SHAPES = [(1, 8, 8), (3, 1000, 1008), (5, 32000, 32000), (2, 128256, 128256), (64, 4096, 4104)]
ODD = (2, 1003, 1008)                    # n % 8 != 0: the last 16-byte unit of a row reaches into the padding
SMALL, MID, BIG, WIDE = SHAPES[1], SHAPES[2], SHAPES[3], SHAPES[4]
CANARY = 65504.0
RANDOM_PARAMS = [(0.8, 0, 1.0), (0.8, 50, 0.9), (1.0, 0, 0.5), (1.3, 7, 1.0)]


def _device_rows(gpu, x):
    """x: numpy fp16 [rows, n] -> a device view [rows, n] of a [rows, stride] buffer whose padding holds canaries."""
    rows, n = x.shape
    stride = {8: 8, 1000: 1008, 1003: 1008, 4096: 4104}.get(n, n)
    buf = torch.full((rows, stride), CANARY, dtype=torch.float16, device=gpu)
    buf[:, :n] = torch.from_numpy(x).to(gpu)
    return buf[:, :n]


def _sample(gpu, x, T=1.0, k=0, p=1.0, u=None, **kw):
    """Run the kernel on numpy rows -> (tokens, uniforms used), numpy.  T, k, p: scalars or numpy [rows]; u: None (generator), a scalar or
    [rows]."""
    from qserve_amd.sampling import sample_rows
    rows, n = x.shape
    xd = _device_rows(gpu, x)
    dev = lambda v, dt: torch.from_numpy(np.asarray(v, dtype=dt)).to(gpu) if isinstance(v, np.ndarray) else v   # noqa: E731
    out = torch.full((rows + 2,), -7, dtype=torch.int64, device=gpu)
    u_out = torch.full((rows,), -1.0, dtype=torch.float32, device=gpu)
    if u is not None:
        u = torch.from_numpy(np.broadcast_to(np.asarray(u, dtype=np.float32), (rows,)).copy()).to(gpu)
    sample_rows(xd, out, dev(T, np.float32), dev(k, np.int32), dev(p, np.float32), uniforms=u, u_out=u_out, **kw)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert out[rows:].tolist() == [-7, -7], "out was written behind `rows`"
    assert ((out[:rows] >= 0) & (out[:rows] < n)).all(), f"a token outside [0, n): {out[:rows]}"
    return out[:rows], u_out.cpu().numpy()


def _argmax(gpu, x):
    from qserve_amd.decode import argmax_rows_
    out = torch.empty((x.shape[0],), dtype=torch.int64, device=gpu)
    argmax_rows_(_device_rows(gpu, x), out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _random(shape, seed, sigma=3.0):
    rows, n, _ = shape
    return (np.random.default_rng(seed).standard_normal((rows, n)) * sigma).astype(np.float16)


@pytest.mark.parametrize("shape", SHAPES + [ODD], ids=str)
@pytest.mark.parametrize("params", RANDOM_PARAMS, ids=str)
def test_random_rows_against_the_oracle(gpu, shape, params):
    T, k, p = params
    x = _random(shape, 100 + shape[1])
    tok, u = _sample(gpu, x, T, k, p, seed=42)
    check_tokens(x, tok, u, T, k, p)
    assert (x[np.arange(x.shape[0]), tok] > -np.inf).all()


def test_per_row_parameter_arrays(gpu):
    rows, n, _ = WIDE
    rng = np.random.default_rng(7)
    x = _random(WIDE, 8)
    x[3, [5, 900, 4000]] = x[3].max()                                # a row with repeated maxima
    T = rng.choice(np.array([0.5, 0.8, 1.0, 2.0, 1e-6], dtype=np.float32), size=rows)
    k = rng.choice(np.array([0, 1, 50, 5000], dtype=np.int32), size=rows)
    p = rng.choice(np.array([1.0, 0.9, 0.5, 1e-9], dtype=np.float32), size=rows)
    tok, u = _sample(gpu, x, T, k, p, seed=3)
    checked = check_tokens(x, tok, u, T, k, p)
    assert sum(r.greedy for r in checked) >= 5 and sum(not r.greedy for r in checked) >= 20
    assert np.array_equal(u, philox_uniform(np.arange(rows), 3))


def _planted(shape):
    """Rows whose survivors are four tokens of mass .4 / .3 / .2 / .1 (in index order): at the first index, on both sides of the boundary
    between the first two wave segments of the kernel's last pass, and at the last index; everything else 20 below."""
    rows, n, _ = shape
    x = np.full((rows, n), -20.0, dtype=np.float16)
    units = (n + 7) // 8
    b = 8 * ((units + 15) // 16)
    pos = [0, b - 1, b, n - 1] if b < n - 1 and b - 1 > 0 else [0, n // 2 - 1, n // 2, n - 1]
    x[:, pos] = np.log(np.array([0.4, 0.3, 0.2, 0.1])).astype(np.float16)
    return x, pos


@pytest.mark.parametrize("shape", [SHAPES[0], SMALL, MID, BIG, ODD], ids=str)
@pytest.mark.parametrize("params", [(1.0, 4, 1.0), (1.0, 0, 0.95)], ids=str)
def test_planted_survivors_at_the_midpoints(gpu, shape, params):
    T, k, p = params
    x, pos = _planted(shape)
    for want, u in zip(pos, (0.2, 0.55, 0.8, 0.95)):
        tok, used = _sample(gpu, x, T, k, p, u=u)
        rows = check_tokens(x, tok, used, T, k, p, equal=True)
        for r in rows:
            assert r.nucleus_margin() >= 0.01 and r.u_margin(u) >= 0.01 and sorted(np.nonzero(r.survivors())[0]) == sorted(pos)
        assert (tok == want).all()


@pytest.mark.parametrize("shape", [SMALL, BIG, ODD], ids=str)
def test_the_ends_of_the_unit_interval(gpu, shape):
    """u = 0 gives the first survivor, u = 1 - 2^-24 the last one - never a non-survivor, never an index out of range."""
    for x, T, k, p in ((_random(shape, 5), 0.8, 50, 1.0), (_random(shape, 6, sigma=1.0), 1.0, 0, 1.0), (_planted(shape)[0], 1.0, 4, 1.0),
                       (_planted(shape)[0], 1.0, 0, 0.95)):
        first, _ = _sample(gpu, x, T, k, p, u=0.0)
        last, _ = _sample(gpu, x, T, k, p, u=U_MAX)
        for r in range(x.shape[0]):
            S = np.nonzero(Row(x[r], T, k, p).survivors())[0]
            assert first[r] == S[0] and last[r] == S[-1], f"row {r}: {first[r]}, {last[r]}, survivors {S[0]} .. {S[-1]}"


@pytest.mark.parametrize("shape", [SMALL, MID, WIDE, ODD], ids=str)
def test_greedy_equivalence(gpu, shape):
    rows, n, _ = shape
    x = _random(shape, 21)
    rep = list(range(0, rows, 2))                                    # every other row: the maximum three times
    for r in range(rows):
        x[r, [n // 3, n // 2, n - 2] if r in rep else [n // 5]] = np.float16(x[r].max() + 1)
    am = _argmax(gpu, x)
    assert all(am[r] == n // 3 for r in rep)
    rng = np.random.default_rng(1)
    u = rng.random(rows).astype(np.float32)
    for T, k, p in ((1e-6, 0, 1.0), (1.0, 0, 1e-9), (1e-6, 1, 1e-9)):          # the greedy conditions, under any u
        tok, _ = _sample(gpu, x, T, k, p, u=u)
        assert np.array_equal(tok, am), (T, k, p)
    tok, _ = _sample(gpu, x, 1.0, 1, 1.0, u=0.0)                                # k = 1: the first maximum at u = 0 ...
    assert np.array_equal(tok, am)
    tok, _ = _sample(gpu, x, 1.0, 1, 1.0, u=u)
    uniq = [r for r in range(rows) if r not in rep]
    assert np.array_equal(tok[uniq], am[uniq])                                   # ... under any u where the maximum is alone ...
    assert all(x[r, tok[r]] == x[r].max() for r in range(rows))                  # ... and always a maximum
    check_tokens(x, tok, u, 1.0, 1, 1.0)
    tok, _ = _sample(gpu, x, 1.0, 0, 1e-6, u=u)                                  # a nucleus of almost nothing: the maximum's class
    assert all(x[r, tok[r]] == x[r].max() for r in range(rows))
    check_tokens(x, tok, u, 1.0, 0, 1e-6)


@pytest.mark.parametrize("shape", [SMALL, MID], ids=str)
def test_filters_that_filter_nothing(gpu, shape):
    rows, n, _ = shape
    x = _random(shape, 31)
    base, u = _sample(gpu, x, 0.8, 0, 1.0, seed=9)
    for k in (n, n + 5, -1):
        tok, u2 = _sample(gpu, x, 0.8, k, 1.0, seed=9)
        assert np.array_equal(tok, base) and np.array_equal(u, u2)
    tok, _ = _sample(gpu, x, 0.8, n, 1.5, seed=9)
    assert np.array_equal(tok, base)
    check_tokens(x, base, u, 0.8, 0, 1.0)


@pytest.mark.parametrize("shape", [MID, BIG, ODD], ids=str)
def test_all_equal_row_is_uniform_over_the_indices(gpu, shape):
    """One class of n members: a count or a mass that overflows shows here.  Ties stay, so no filter removes anything."""
    rows, n, _ = shape
    x = np.full((rows, n), 1.5, dtype=np.float16)
    u = np.random.default_rng(2).random(rows).astype(np.float32)
    for T, k, p in ((0.7, 0, 1.0), (0.7, 5, 1.0), (1.0, 0, 0.5), (100.0, 3, 0.1)):
        tok, used = _sample(gpu, x, T, k, p, u=u)
        check_tokens(x, tok, used, T, k, p)
        assert (np.abs(tok - np.floor(u.astype(np.float64) * n)) <= np.ceil(DELTA * n)).all(), (tok, u * n)


@pytest.mark.parametrize("shape", [SMALL, MID, BIG], ids=str)
@pytest.mark.parametrize("T", [100.0, 1e-3], ids=str)
def test_extreme_temperatures(gpu, shape, T):
    """T = 100: all weights near 1, W near n.  T = 1e-3: all weights but a few underflow."""
    x = _random(shape, 41)
    for k, p in ((0, 1.0), (50, 0.9)):
        tok, u = _sample(gpu, x, T, k, p, seed=5)
        check_tokens(x, tok, u, T, k, p)


@pytest.mark.parametrize("shape", [SHAPES[0], SMALL, BIG], ids=str)
def test_masked_rows(gpu, shape):
    rows, n, _ = shape
    x = np.full((rows, n), -np.inf, dtype=np.float16)
    live = [1, n // 2, n - 1]
    x[:, live] = np.array([0.5, 1.25, -0.75], dtype=np.float16)
    for k, p, seed in ((0, 1.0, 1), (0, 1.0, 2), (2, 1.0, 3), (0, 0.7, 4), (n - 1, 0.999, 5)):
        tok, u = _sample(gpu, x, 1.0, k, p, seed=seed)
        assert all(t in live for t in tok)
        check_tokens(x, tok, u, 1.0, k, p)
    for u in (0.0, 0.5, U_MAX):
        tok, used = _sample(gpu, x, 2.0, 0, 1.0, u=u)
        assert all(t in live for t in tok)
        check_tokens(x, tok, used, 2.0, 0, 1.0)


@pytest.mark.parametrize("shape", [SMALL, WIDE], ids=str)
def test_generator_is_philox_bit_for_bit(gpu, shape):
    from qserve_amd.sampling import position_keys as device_keys
    rows, n, _ = shape
    x = _random(shape, 51)
    for seed in (0, 12345, (1 << 63) + 0x1234567):
        _, u = _sample(gpu, x, seed=seed)                                        # row_keys null: the key is the row index
        assert np.array_equal(u, philox_uniform(np.arange(rows), seed))
        seq = np.random.default_rng(seed % 1000).integers(0, 1 << 20, size=rows)
        pos = np.random.default_rng(seed % 1000 + 1).integers(0, 1 << 31, size=rows)
        keys = device_keys(torch.from_numpy(seq).to(gpu), torch.from_numpy(pos).to(gpu).to(torch.int32))
        assert keys.dtype == torch.int64 and np.array_equal(keys.cpu().numpy(), position_keys(seq, pos))
        tok, u = _sample(gpu, x, 0.9, seed=seed, row_keys=keys)
        assert np.array_equal(u, philox_uniform(position_keys(seq, pos), seed))
        assert ((u >= 0) & (u < 1)).all()
        check_tokens(x, tok, u, 0.9)


@pytest.mark.parametrize("shape", [SMALL, MID], ids=str)
def test_uniforms_override_the_generator(gpu, shape):
    rows, n, _ = shape
    x = _random(shape, 61)
    u = np.random.default_rng(3).random(rows).astype(np.float32)
    tok, used = _sample(gpu, x, 0.8, 40, 0.95, u=u, seed=77)
    assert np.array_equal(used, u)
    check_tokens(x, tok, u, 0.8, 40, 0.95)
    tok2, used2 = _sample(gpu, x, 0.8, 40, 0.95, u=u, seed=78)                  # the seed plays no part
    assert np.array_equal(tok, tok2) and np.array_equal(used2, u)


@pytest.mark.parametrize("shape", [SMALL, BIG, WIDE], ids=str)
def test_deterministic_and_capturable(gpu, shape):
    """The same call twice: bit-equal.  Captured and replayed twice: equal to eager.  A replay after an in-graph change of row_keys draws
    other uniforms - the ones of the new keys."""
    from qserve_amd.sampling import sample_rows
    rows, n, _ = shape
    x = _random(shape, 71)
    xd = _device_rows(gpu, x)
    keys0 = torch.arange(rows, dtype=torch.int64, device=gpu) * 7 + 100
    kw = dict(temperature=0.8, top_k=50, top_p=0.9, seed=11)
    eager = [sample_rows(xd, row_keys=keys0, **kw).clone() for _ in range(2)]
    assert torch.equal(eager[0], eager[1])
    out, out_b = torch.zeros_like(eager[0]), torch.zeros_like(eager[0])
    u_b = torch.zeros((rows,), dtype=torch.float32, device=gpu)
    keys = keys0.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sample_rows(xd, out, row_keys=keys0, **kw)
        keys.add_(1)                                                             # the in-graph change of the keys
        sample_rows(xd, out_b, row_keys=keys, u_out=u_b, **kw)
    seen = []
    for i in range(2):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager[0]), f"replay {i} differs from the eager call"
        want = philox_uniform(keys0.cpu().numpy() + i + 1, 11)
        assert np.array_equal(u_b.cpu().numpy(), want), f"replay {i}: not the uniforms of the advanced keys"
        check_tokens(x, out_b.cpu().numpy(), want, 0.8, 50, 0.9)
        seen.append(u_b.cpu().numpy().copy())
    assert not np.array_equal(seen[0], seen[1])
    check_tokens(x, eager[0].cpu().numpy(), philox_uniform(keys0.cpu().numpy(), 11), 0.8, 50, 0.9)


def test_wrapper_rejects_what_the_kernel_cannot_take(gpu):
    from qserve_amd.sampling import sample_rows
    x = torch.zeros((4, 64), dtype=torch.float16, device=gpu)
    with pytest.raises(RuntimeError):
        sample_rows(x.float())
    with pytest.raises(RuntimeError):
        sample_rows(x[:, :7])
    with pytest.raises(RuntimeError):
        sample_rows(x[:, ::2])
    with pytest.raises(RuntimeError):
        sample_rows(torch.zeros((4, 33), dtype=torch.float16, device=gpu))        # a row stride that is no multiple of 8
    with pytest.raises(RuntimeError):
        sample_rows(x, temperature=torch.ones((3,), dtype=torch.float32, device=gpu))
    with pytest.raises(RuntimeError):
        sample_rows(x, out=torch.zeros((4,), dtype=torch.int32, device=gpu))
    with pytest.raises(RuntimeError):
        sample_rows(x, row_keys=torch.zeros((4,), dtype=torch.int64))               # on the host
    assert sample_rows(x[:0]).numel() == 0


def test_most_random_cases_admit_one_survivor_set():
    """The condition on the inputs of test_random_rows_against_the_oracle, on the oracle alone."""
    single = []
    for shape in SHAPES + [ODD]:
        x = _random(shape, 100 + shape[1])
        for T, k, p in RANDOM_PARAMS:
            single.extend(len(Row(x[r], T, k, p).candidates()) == 1 for r in range(x.shape[0]))
    assert len(single) >= 300 and sum(single) >= 0.9 * len(single), f"only {sum(single)} of {len(single)} cases have one admissible set"
