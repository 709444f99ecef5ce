"""The float64 oracle of `qs_logprob_rows` (include/qserve_amd.h): log-softmax, rank and top list by a stable sort on (key, index), and
the slot rule - which row a slot reads, which id it scores, which column it writes - restated from the header.  Shared by
tests/test_logprob_rows_*.py and tests/test_logprobs_engine_gpu.py."""
import numpy as np

# |lp - exact| <= ABS + REL * |lp|, lp = (a_t - (log2(float(W)) - 40)) * ln 2 in the kernel's fp32 arithmetic against the float64
# log-softmax.  Absolute terms, in nats (W >= 2^40: the maximum's own weight):
#   fixed-point truncation   each of n <= 2^22 weights loses < 1 of W >= 2^40: < n * 2^-40 <= 2^-18 of W       3.8e-6
#   float(W)                 one fp32 rounding, 2^-24 of W                                                       6.0e-8
#   exp2                     ~1 ulp per weight, 2^-23 of W at the worst                                          1.2e-7
#   log2                     ~1 ulp of a result in [40, 62): 2^-18, times ln 2 (the - 40 is exact;
#                            what is left, log2 W - 40 <= 22, keeps that spacing)                               2.6e-6
#                            sum 6.6e-6, rounded up to 1e-5.
# Terms proportional to |lp| (|a_t| * ln 2 <= |lp|, because log2 W - 40 >= 0): x_t - m, its product with the scale and the rounding of
# the scale itself, 2^-24 each on a_t; the difference a_t - lg, ln 2 as a float (2^-25) and the last product: 2^-24 each on lp -
# together below 6 * 2^-24 * |lp|, rounded up to 2^-21 = 8 * 2^-24.
ABS, REL = 1e-5, 2.0 ** -21


def TOL(lp):
    return ABS + REL * np.abs(lp)


def keys(x):
    """fp16 [..] -> the order-preserving 16-bit key of every value as int64 (-0 is +0)."""
    assert x.dtype == np.float16
    b = x.view(np.uint16).astype(np.int64)
    b = np.where(b == 0x8000, 0, b)
    return np.where(b & 0x8000, b ^ 0xFFFF, b ^ 0x8000)


def temperature(T):
    """The T the contract uses for the float32 parameter T: below 1e-5 (greedy) it is 1."""
    T = np.float32(T)
    return 1.0 if not T >= np.float32(1e-5) else float(T)


def log_softmax(x, T=1.0):
    """float64 log softmax(x / T) of one fp16 row (-inf logits give -inf)."""
    z = x.astype(np.float64) / temperature(T)
    z = z - z.max()
    with np.errstate(divide="ignore"):
        return z - np.log(np.exp(z).sum())


def order(x):
    """The ids of the row in the order (key descending, index ascending)."""
    return np.argsort(-keys(x), kind="stable")


def score(x, t, T=1.0, top=0):
    """One row, one id -> (lp float64, rank int, top ids int list, top lps float64 list) by the contract."""
    n = x.size
    lsm = log_softmax(x, T)
    o = order(x)
    listed = o[x[o] != -np.inf][:top].tolist()
    ids = listed + [-1] * (top - len(listed))
    lps = [float(lsm[i]) for i in listed] + [-np.inf] * (top - len(listed))
    if not 0 <= t < n:
        return np.nan, 0, ids, lps
    return float(lsm[t]), int(np.nonzero(o == t)[0][0]) + 1, ids, lps


def slots(node_tokens, accept_idx, accept_lens, next_token, lengths, batch, n, max_accept, out_cols):
    """The slot rule -> [(b, j, logits row, id, column)] of every slot that writes.  Arrays as the entry takes them, or None."""
    res = []
    clamp = lambda i: min(max(int(i), 0), n - 1)   # noqa: E731
    for b in range(batch):
        cap = max_accept if node_tokens is not None and accept_idx is not None else 1
        m = 1 if accept_lens is None else min(max(int(accept_lens[b]), 0), cap)
        for j in range(1, m + 1):
            row = b * n + (clamp(accept_idx[b, j - 1]) if accept_idx is not None else 0)
            t = int(node_tokens[b, clamp(accept_idx[b, j])]) if j < m else int(next_token[b])
            col = j - 1 if lengths is None else max(int(lengths[b]), 0) - 1 + j
            if col < out_cols:
                res.append((b, j, row, t, col))
    return res


NAN_LP, NO_RANK, NO_ID = np.float32(np.nan), 0, -1        # what a fresh log holds


def expected_logs(x, written, T, top, batch, cols):
    """x fp16 [rows, n]; written: the list of `slots`; T a scalar or [batch] -> the float64 / int arrays a fresh set of logs holds
    after the launch: (lp [batch, cols], rank, top_ids [batch, cols, top], top_lp), NaN / 0 / -1 / NaN where no slot wrote."""
    lp = np.full((batch, cols), np.nan)
    rank = np.zeros((batch, cols), dtype=np.int64)
    ids = np.full((batch, cols, top), -1, dtype=np.int64)
    tlp = np.full((batch, cols, top), np.nan)
    Ts = np.broadcast_to(np.asarray(T, dtype=np.float32), (batch,))
    for b, _, row, t, col in written:
        lp[b, col], rank[b, col], i, l = score(x[row], t, Ts[b], top)
        ids[b, col], tlp[b, col] = i, l
    return lp, rank, ids, tlp


def assert_close(got, want, what):
    """float32 results against float64 expectations: NaN where NaN, -inf where -inf, else within TOL."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN pattern differs"
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf]), f"{what}: infinities differ"
    ok = ~inf & ~np.isnan(want)
    err = np.abs(got[ok] - want[ok])
    bad = err > TOL(want[ok])
    worst = float((err / TOL(want[ok])).max()) if err.size else 0.0
    print(f"{what}: {err.size} values, worst error {worst:.3f} of the bound")
    assert not bad.any(), f"{what}: {int(bad.sum())} values beyond TOL, worst {worst:.3f} of the bound ({got[ok][bad][:4]} vs {want[ok][bad][:4]})"
    return worst
