"""One construction for every long-context attention test (tests/test_long_positions_cpu.py pins it on the host,
tests/test_long_positions_gpu.py runs it): a context of tens of thousands of tokens that costs 8 pages of K / V.

A sequence with `past` cached tokens has a pointer table of `mb` entries.  Its past // 64 full pages ALIAS R = 8 physical pages: entry j
names physical page (8 * j) // (past // 64), so eighth e of the context reads page e over and over.  The 8 pages (and one "tail" page
per sequence) are written ONCE by the existing prefill writer from `Case.hist` - on the device by the GPU tests, by its numpy oracle on
the host; their bytes are what they are, and the float64 reference reads the same bytes (tests/_append_cases.py).  The partial last
page of a sequence is its own tail page (physical page 8 + b, of which the first past % 64 tokens count), the pages behind it that can
receive new tokens are fresh pages of the sequence's own, every other entry names one dummy page, and one spare page belongs to nobody.
K and V pools number their pages independently (V page = vperm[K page]).

K and q are standard normal.  V of physical page p is N(0, 1) + C * sign[p, d]: an offset per (page, dimension).  Plain normal values
at 33 000 keys average out to about 0.01, where the 2e-3 bar of the fp16 attention tests would pass a kernel that loses a whole split;
with the offsets, removing an eighth of the context moves every dimension by about C / 7.  The signs of the 8 history pages are balanced
per dimension (4 + / 4 -, shuffled per dimension): the offsets cancel in the full result, whose size then comes from the unequal
softmax weights of the pages alone - a page is the same 64 keys read again and again, so its weight strays from 1 / 8 by some 15 % -,
about 0.3 C at the largest element.  C = 2.3 is the window between two conditions: the SHORTEST page range a launch uses as a split
- 64 forced splits over 516 pages are 57 ranges of 9 pages and one of 2 pages + 40 tokens, 0.5 % of the context - must still move the
result by 5 x TOL = 0.01, about 0.005 x C, while max |reference| must stay below 1 (values measured at 33 000 tokens: shortest range
0.0109 .. 0.0128, max |reference| 0.50 .. 0.72; tests/test_long_positions_cpu.py prints them).

`conditions` states what the GPU tests rely on, on the float64 reference over the QUANTISED pages:
    * removing any eighth of the past moves every (row, head) by >= SENS x TOL (tests/_attn_cases.py SENS),
    * removing any page range a launch uses as a split moves every (row, head) by >= 5 x TOL,
    * max |reference| < 1."""
import numpy as np

from _append_cases import compose
from oracle import kvattn

R = 8                      # physical history pages
C = 2.3
TOL = 2e-3                 # tests/test_append_gpu.py: an fp16 attention against the float64 oracle on O(1) outputs
LONGEST = 2046 * 64 + 40   # 130 984 tokens (2047 pages, table of 2048): one float64 reference takes a few seconds (test_long_positions_cpu.py)
LONG = 515 * 64 + 40       # 33 000 tokens: 516 pages, not a multiple of 64 tokens


def signs(rng, ntail):
    """+-1 [R + ntail, 128]: history pages balanced per dimension (four of each sign), tail pages free."""
    s = np.stack([rng.permutation(np.asarray([1, 1, 1, 1, -1, -1, -1, -1], np.float32)) for _ in range(128)], axis=1)
    return np.concatenate([s, rng.choice(np.asarray([-1.0, 1.0], np.float32), size=(ntail, 128))])


class Case:
    """pasts: cached tokens per sequence (1 or 2 sequences), ns: new rows per sequence, mb: pointer table entries.
    shared_pages: sequence 1's first entries are sequence 0's (a shared prefix of that many pages)."""

    def __init__(self, H, Hkv, int4, pasts, ns, mb, seed, c=C, shared_pages=0):
        r = np.random.default_rng(seed)
        self.H, self.Hkv, self.int4, self.mb, self.c = H, Hkv, int4, mb, c
        self.B, self.W, self.spt = len(pasts), (H + 2 * Hkv) * 128, Hkv * (64 if int4 else 128)
        self.past, self.ns = np.asarray(pasts, np.int32), list(ns)
        self.cu_q = np.concatenate([[0], np.cumsum(ns)]).astype(np.int32)
        self.T = int(self.cu_q[-1])
        B = self.B
        assert all(0 < p and (p + n + 63) // 64 <= mb for p, n in zip(pasts, ns))
        # physical pages (K numbering): 0 .. 7 history, 8 + b tails, then each sequence's fresh pages, the dummy, the spare
        nxt = R + B
        tab = np.zeros((B, mb), np.int64)
        fresh = []
        for b, (p, n) in enumerate(zip(pasts, ns)):
            full = p // 64
            tab[b, :full] = (R * np.arange(full)) // full
            tab[b, full] = R + b
            last = max(p + n - 1, p) // 64
            for j in range(full + 1, last + 1):
                tab[b, j] = nxt
                fresh.append(nxt)
                nxt += 1
            tab[b, last + 1:] = -1
        if shared_pages:
            assert B == 2 and shared_pages <= min(pasts) // 64
            tab[1, :shared_pages] = tab[0, :shared_pages]
        self.dummy, self.spare, self.nblocks = nxt, nxt + 1, nxt + 2
        tab[tab < 0] = self.dummy
        self.vperm = r.permutation(self.nblocks).astype(np.int64)
        self.tables = np.stack([tab, self.vperm[tab]], axis=1)                       # [B, 2, mb]
        self.hist_tables = np.stack([np.arange(R + B), self.vperm[: R + B]])[None].astype(np.int64)      # the prefill call's table [1, 2, 8 + B]
        self.hist_len = (R + B) * 64
        self.sign = signs(r, B)
        hist = r.standard_normal((self.hist_len, self.W)).astype(np.float32)
        v = hist[:, (H + Hkv) * 128:].reshape(R + B, 64, Hkv, 128)
        v += c * self.sign[:, None, None, :]
        self.hist = hist.astype(np.float16)
        self.new = r.standard_normal((self.T, self.W)).astype(np.float16)

    def host_pages(self, base):
        """The oracle's prefill writer over `hist`: a 0xFF-filled PagePool holding the 8 + B written pages."""
        pool = kvattn.PagePool(self.nblocks, self.Hkv, 128, self.int4, fill=0xFF)
        rows = self.hist.copy()
        kvattn.prefill_update_kv_cache(rows, np.asarray([self.hist_len], np.int32), np.zeros(self.hist_len, np.int32), self.hist_tables, pool,
                                       self.H, self.Hkv, self.hist_len, base)
        return pool


def eighths(past):
    return [(e * past // 8, (e + 1) * past // 8) for e in range(8)]


def split_ranges(past, splits, page0=0):
    """Token ranges of the non-empty page ranges `split_range` (csrc/append_walk.h) cuts the pages from `page0` on into:
    ceil(pages / splits) pages per split."""
    np_all = (past - page0 * 64 + 63) // 64
    pps = (np_all + splits - 1) // splits
    out = []
    for s in range(splits):
        p0 = min(s * pps, np_all)
        npg = pps if p0 + pps < np_all else np_all - p0
        if npg > 0:
            out.append(((page0 + p0) * 64, min((page0 + p0 + npg) * 64, past)))
    return out


class Reference:
    """float64 attention of ONE sequence of the composed problem with removable key ranges: row i sees keys 0 .. past + i (or, with
    `words`, the cached keys and the new keys its word names).  Un-normalised weights are kept, so removing a range costs one pass
    over that range."""

    def __init__(self, q, K, V, past, words=None):
        n, H, _ = q.shape
        G = H // K.shape[1]
        self.past, self.n, self.H, self.G = past, n, H, G
        self.V = V.astype(np.float64)
        K64 = K.astype(np.float64)
        S = np.stack([q[:, h].astype(np.float64) @ K64[:, h // G].T for h in range(H)]) / np.sqrt(128.0)      # [H, n, L]
        vis = np.ones((n, past + n), bool)
        if words is None:
            vis[:, past:] = np.tril(np.ones((n, n), bool))
        else:
            vis[:, past:] = [[(int(w) >> j) & 1 == 1 for j in range(n)] for w in words]
        S = np.where(vis[None], S, -np.inf)
        self.P = np.exp(S - S.max(axis=2, keepdims=True))                 # [H, n, L]
        self.num, self.den = self._sums(0, past + n)
        self.out = (self.num / self.den[..., None]).transpose(1, 0, 2)   # [n, H, 128]

    def _sums(self, a, e):
        num = np.stack([self.P[h, :, a:e] @ self.V[a:e, h // self.G] for h in range(self.H)])
        return num, self.P[:, :, a:e].sum(axis=2)

    def moved_without(self, a, e):
        """min over (row, head) of max over dims |out without keys a .. e - 1  -  out|."""
        num, den = self._sums(a, e)
        alt = ((self.num - num) / (self.den - den)[..., None]).transpose(1, 0, 2)
        return float(np.abs(alt - self.out).max(axis=2).min())


def references(case, qkv_rot, pool, words=None):
    """-> ([Reference per sequence], float32 [T, H, 128]) over `pool` (host PagePool: only positions < past are read)."""
    q, K, V, cu_k = compose(qkv_rot, case.cu_q, case.past, case.tables, pool, case.H, case.Hkv)
    refs = []
    for b in range(case.B):
        s, e = int(case.cu_q[b]), int(case.cu_q[b + 1])
        refs.append(Reference(q[s:e], K[cu_k[b]:cu_k[b + 1]], V[cu_k[b]:cu_k[b + 1]], int(case.past[b]),
                              None if words is None else words[s:e]))
    return refs, np.concatenate([r.out for r in refs]).astype(np.float32)


def conditions(case, refs, split_sets, what, sens):
    """The three host conditions; split_sets: per sequence a list of token ranges the launch under test uses as splits."""
    for b, ref in enumerate(refs):
        e8 = min(ref.moved_without(a, e) for a, e in eighths(ref.past))
        sp = min([ref.moved_without(a, e) for a, e in split_sets[b]], default=float("inf"))
        mx = float(np.abs(ref.out).max())
        print(f"{what} seq {b} past {ref.past}: eighth removed moves >= {e8:.4f} (bar {sens * TOL:.3f}), one of {len(split_sets[b])} "
              f"split ranges removed moves >= {sp:.4f} (bar {5 * TOL:.3f}), max |ref| {mx:.3f}")
        assert e8 >= sens * TOL, (what, b, e8)
        assert sp >= 5 * TOL, (what, b, sp)
        assert mx < 1.0, (what, b, mx)


# ---- the cases of tests/test_long_positions_gpu.py (their host conditions: tests/test_long_positions_cpu.py) ------------------------
BASE = 1e6                 # Mistral / Qwen checkpoints
SHARED_PAGES = 256
SHARED_SPLITS = 8          # forced prefix and suffix split counts of the shared-prefix launch (the ranges the conditions are stated for)
SEEDS = {}                 # (kind, H, Hkv, int4, length) -> seed, where the default seed misses a host condition


def append_case(H, Hkv, int4, longest):
    """Two sequences with 8 new rows each over the same number of full pages - past 33 000 (516 pages, table of 520) or LONGEST (2047
    pages, table of 2048) -, so their aliased entries agree (the shared-prefix launch reads the first 256 through sequence 0's table);
    the second one's own last page holds 60 tokens, and its new rows cross into a fresh page."""
    past0, mb = (LONGEST, 2048) if longest else (LONG, 520)
    seed = SEEDS.get(("append", H, Hkv, int4, past0), 100 + 8 * H + 2 * Hkv + int(int4) + 50 * int(longest))
    return Case(H, Hkv, int4, [past0, past0 // 64 * 64 + 60], [8, 8], mb, seed, shared_pages=SHARED_PAGES)


def append_split_sets(case, plan_splits=()):
    """Per sequence: every token range one of the append-family launches of the GPU tests uses as a split - 8 and 64 forced, the
    planner's counts, and the shared-prefix launch's SHARED_SPLITS prefix and suffix ranges."""
    out = []
    for p in case.past.tolist():
        r = [x for n in (8, 64) + tuple(plan_splits) for x in split_ranges(p, n)]
        out.append(r + split_ranges(SHARED_PAGES * 64, SHARED_SPLITS) + split_ranges(p, SHARED_SPLITS, page0=SHARED_PAGES))
    return out


def decode_case(int4, L):
    """single_query_attention at context length L (the new token included), 8 / 2 heads: two sequences of L and L - 70 tokens, one at the
    longest length; the pointer table holds exactly the pages of L."""
    B = 1 if L > 40000 else 2
    seed = SEEDS.get(("decode", 8, 2, int4, L), 300 + int(int4) + L % 1000)
    return Case(8, 2, int4, [L - 1, L - 71][:B], [1] * B, (L + 63) // 64, seed)


def decode_split_ranges(past, nsplit, int4):
    """The cached-token ranges of the matrix-core decode kernels' KV splits (tests/_attn_cases.py split_boundaries)."""
    import _attn_cases as AC
    b = AC.split_boundaries(past + 1, nsplit, int4)
    return [(b[i], b[i + 1] + 1) for i in range(0, len(b), 2)]
