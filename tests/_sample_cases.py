"""The float64 oracle of `qs_sample_rows` (include/qserve_amd.h: the per-row semantics in exact arithmetic), a numpy Philox4x32-10, the
acceptance rule the GPU tests apply to the kernel's tokens, and the host walk of sampled tree verification.  Shared by
tests/test_sample_rows_*.py and tests/test_sampled_verify_gpu.py."""
import numpy as np

DELTA = 1e-4            # tolerance in normalised cumulative probability: <= 1024-term fp32 chains + a <= 20-level tree at 2^-24 per
#                         addition and ~1 ulp of the exponential give ~6.3e-5, rounded up
U_MAX = 1.0 - 2.0 ** -24

_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter [..., 4], key [..., 2] (uint32 values) -> uint32 [..., 4]: Philox4x32 with 10 rounds, written from the published round
    function."""
    c = [np.asarray(counter)[..., i].astype(np.uint64) for i in range(4)]
    k = [np.asarray(key)[..., i].astype(np.uint64) for i in range(2)]
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & _MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & _MASK]
        k = [(k[0] + np.uint64(_W0)) & _MASK, (k[1] + np.uint64(_W1)) & _MASK]
    return np.stack(c, axis=-1).astype(np.uint32)


def philox_uniform(keys, seed):
    """The uniform `qs_sample_rows` draws for the int64 `keys` under `seed`: counter (key_lo, key_hi, 0, 0), key (seed_lo, seed_hi),
    first word, (word >> 8) * 2^-24 -> float32 array."""
    keys = np.asarray(keys, dtype=np.int64).astype(np.uint64)
    ctr = np.stack([keys & _MASK, keys >> np.uint64(32), np.zeros_like(keys), np.zeros_like(keys)], axis=-1)
    seed = int(seed)
    key = np.broadcast_to(np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64), ctr.shape[:-1] + (2,))
    word = philox4x32_10(ctr, key)[..., 0]
    return ((word >> np.uint32(8)).astype(np.float64) * 2.0 ** -24).astype(np.float32)


def position_keys(seq_ids, positions):
    return (np.asarray(seq_ids, dtype=np.int64) << 32) | np.asarray(positions, dtype=np.int64)


class Row:
    """The exact semantics of one row.  x: fp16 [n]; T, p as the float32 values the kernel receives; k int.
    .greedy, .argmax;  .classes(): value classes in descending order with their tail masses;  .survivors(v_p) -> mask for a nucleus value
    threshold;  .exact_threshold;  .token(u);  .candidates(): the thresholds the acceptance rule admits;  .accepts(t, u)."""

    def __init__(self, x, T=1.0, k=0, p=1.0):
        assert x.dtype == np.float16 and x.ndim == 1
        self.x = x.astype(np.float64)
        self.n = x.size
        self.T, self.p, self.k = np.float32(T), np.float32(p), int(k)
        self.argmax = int(np.argmax(self.x))                       # first maximum
        self.greedy = bool(self.T < np.float32(1e-5) or self.p < np.float32(1e-8))
        if self.greedy:
            return
        with np.errstate(over="ignore", invalid="ignore"):
            self.w = np.exp((self.x - self.x.max()) / float(self.T))
        self.W = self.w.sum()
        vals, inv = np.unique(self.x, return_inverse=True)         # ascending
        mass = np.bincount(inv, weights=self.w, minlength=vals.size)
        self.vals, self.tail = vals[::-1], np.cumsum(mass[::-1])    # descending values, mass of everything >= the value
        self.tau_k = -np.inf
        if 0 < self.k < self.n:
            self.tau_k = np.partition(self.x, self.n - self.k)[self.n - self.k]     # the k-th largest logit
        if self.p >= 1:
            self.exact = self.vals.size - 1                         # every value survives the nucleus
        else:
            self.exact = int(np.argmax(self.tail >= float(self.p) * self.W))

    def nucleus_margin(self):
        """The distance of p * W from the nearest class boundary of the tail mass, as a fraction of W (inf with the nucleus off)."""
        if self.greedy or self.p >= 1:
            return np.inf
        return float(np.min(np.abs(self.tail - float(self.p) * self.W)) / self.W)

    def candidates(self):
        """Indices (into the descending value classes) of the admissible nucleus thresholds: the exact one, and every one whose tail mass
        is within DELTA * W of p * W."""
        if self.p >= 1:
            return [self.exact]
        near = np.nonzero(np.abs(self.tail - float(self.p) * self.W) <= DELTA * self.W)[0].tolist()
        return sorted(set(near) | {self.exact})

    def survivors(self, cls=None):
        v_p = self.vals[self.exact if cls is None else cls]
        return self.x >= max(v_p, self.tau_k)

    def cdf(self, cls=None):
        """-> (mask S, cdf_lo, cdf_hi): normalised cumulative probability over the survivors in index order."""
        S = self.survivors(cls)
        ws = np.where(S, self.w, 0.0)
        hi = np.cumsum(ws)
        WS = hi[-1]
        return S, (hi - ws) / WS, hi / WS

    def token(self, u):
        if self.greedy:
            return self.argmax
        S = self.survivors()
        ws = np.where(S, self.w, 0.0)
        cum = np.cumsum(ws)
        hit = np.nonzero(S & (cum > float(u) * cum[-1]))[0]
        return int(hit[0]) if hit.size else int(np.nonzero(S)[0][-1])

    def u_margin(self, u):
        """The distance of u from the CDF edges of the exact token."""
        t = self.token(u)
        _, lo, hi = self.cdf()
        return min(float(u) - lo[t], hi[t] - float(u))

    def accepts(self, t, u):
        """The acceptance rule: for some admissible survivor set, t is in it and CDF_lo(t) - DELTA <= u < CDF_hi(t) + DELTA."""
        t = int(t)
        if not 0 <= t < self.n:
            return False
        if self.greedy:
            return t == self.argmax
        for c in self.candidates():
            S, lo, hi = self.cdf(c)
            if S[t] and lo[t] - DELTA <= float(u) < hi[t] + DELTA:
                return True
        return False


def check_tokens(x, tokens, us, T=1.0, k=0, p=1.0, equal=False):
    """Every row's kernel token against the oracle -> the oracle rows.  x fp16 [rows, n] (numpy), tokens / us [rows]; T, k, p scalars or
    [rows].  equal=True: the token must be the oracle's (planted cases with margins); otherwise the acceptance rule."""
    rows = []
    par = [np.broadcast_to(np.asarray(v), (x.shape[0],)) for v in (T, k, p)]
    for r in range(x.shape[0]):
        row = Row(x[r], par[0][r], par[1][r], par[2][r])
        t, u = int(tokens[r]), float(us[r])
        if equal:
            assert t == row.token(u), f"row {r}: token {t}, oracle {row.token(u)} (u={u}, T={row.T}, k={row.k}, p={row.p})"
        else:
            assert row.accepts(t, u), f"row {r}: token {t} not admissible, oracle {row.token(u)} (u={u}, T={row.T}, k={row.k}, p={row.p})"
        rows.append(row)
    return rows


def walk(parents, tokens, sampled):
    """The host walk of tree verification for one sequence: from the root, descend to the lowest child whose token equals the token
    sampled at the current node -> (path, bonus token)."""
    n = len(parents)
    path, cur = [0], 0
    while True:
        nxt = next((c for c in range(cur + 1, n) if parents[c] == cur and tokens[c] == sampled[cur]), None)
        if nxt is None:
            return path, int(sampled[cur])
        path.append(nxt)
        cur = nxt


def depths(parents):
    d = []
    for i, p in enumerate(parents):
        d.append(0 if i == 0 else d[p] + 1)
    return d
