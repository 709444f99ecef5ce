"""Launch boundaries and extreme rows for the activation row kernels (qserve_amd/csrc/fused_small.hip, row_ops.h): width tables,
the launchers' selection rules restated, and the row generators.  Pure numpy (no torch, no GPU).
tests/test_row_extremes_cpu.py proves on the CPU that every table follows from the constants the sources state today, that every
instantiation a launcher can select is reached, and that the rows are what they claim; tests/test_row_extremes_gpu.py runs them.
The complement of tests/test_fused_gpu.py, whose Gaussian rows at model widths never put a maximum into a partial last chunk,
never overflow, never meet a rounding tie on purpose and launch 2 of the 5 quantiser geometries.

Every row is fp16.  A BATCH is what one launch gets: T = 3 .. 8 rows.  The GPU test places the outputs of a launch (int8 rows,
scales, sums) inside sentinel-filled stores with one guard row / guard scalar on either side (SENTINEL_*).
"""
import collections

import numpy as np

# ---- the constants of the launchers (tests/test_row_extremes_cpu.py parses the same out of the sources and compares) ------------------
TPB = 256                # fused_small.hip: threads per workgroup of every row kernel but the wide quantisers
WIDE_NT = 1024           # fused_small.hip QS_Q / QS_S: threads of the wide quantiser geometries
WIDE_ROW = 4096          # row_ops.h: rows wider than this take the 1024-thread layout (invoke_quant and silu_and_mul_quant alike)
CHUNK = 8                # fp16 values per 16-byte access; every width is a multiple
BLOCK = 512              # row_ops.h reduce_max_blocksum: the row sum is defined over 512-element blocks
QUANT_MAX = 32768        # qs_invoke_quant / qs_silu_and_mul_quant: widest row
NORM_MAX = 8 * TPB * 8   # qs_rms_norm_general / qs_add_residual_rms_norm_general: widest row (NC = 8)
PLANES_MAX = 2 * TPB * 8  # qs_add_residual_rms_norm_general_planes: widest row (NC = 2)
SILU_MAX_CHUNKS = 16     # qs_silu_and_mul: grid.y is capped here, so one trip of the column loop covers 16 * TPB * 8 columns
RESADD_MAX_BLOCKS = 2048  # qs_residual_add: the grid is capped here, so one trip of the grid-stride loop covers 2048 * TPB * 8 values
ROW = TPB * CHUNK        # 2048: what 256 threads hold with one chunk each

SENTINEL_I8 = 0x5A
SENTINEL_F16_BITS = 0x5A5A      # 203.25: no result of any case below


# ---- which kernel instantiation a launcher selects (restated from the launchers; the CPU test checks the restatement's constants) ----
def quant_inst(h):
    """qs_invoke_quant / qs_silu_and_mul_quant -> (NC, NT) of quant_kernel / silu_mul_quant_kernel."""
    assert 0 < h <= QUANT_MAX and h % CHUNK == 0
    if h > WIDE_ROW:
        return (1 if h <= 8192 else 2 if h <= 16384 else 4, WIDE_NT)
    return (1 if -(-h // ROW) == 1 else 2, TPB)


def _norm_nc(h):
    return {1: 1, 2: 2, 3: 4, 4: 4}.get(-(-h // ROW), 8)


def norm_inst(h, refsum):
    """qs_rms_norm_general -> (NC, REFSUM) of general_norm_quant_kernel.  refsum = row-sum order 1 AND a sum is asked for."""
    assert 0 < h <= NORM_MAX and h % CHUNK == 0
    return (_norm_nc(h), bool(refsum))


def add_norm_inst(h, refsum):
    """qs_add_residual_rms_norm_general -> (NC, FULL, REFSUM) of add_residual_norm_quant_kernel (REFSUM is never FULL)."""
    nc = _norm_nc(h)
    return (nc, (not refsum) and h == nc * ROW, bool(refsum))


def planes_inst(h, ks, per_group, refsum):
    """qs_add_residual_rms_norm_general_planes -> (NC, KS, MODE, FULL, REFSUM) of add_residual_norm_quant_planes_kernel."""
    assert 0 < h <= PLANES_MAX and h % CHUNK == 0 and ks in (1, 2, 4)
    nc = 1 if -(-h // ROW) == 1 else 2
    return (nc, ks, 1 if per_group else 0, (not refsum) and h == nc * ROW, bool(refsum))


ALL_QUANT_INST = {(1, TPB), (2, TPB), (1, WIDE_NT), (2, WIDE_NT), (4, WIDE_NT)}
ALL_NORM_INST = {(nc, r) for nc in (1, 2, 4, 8) for r in (False, True)}
ALL_ADD_NORM_INST = {(nc, f, r) for nc in (1, 2, 4, 8) for f, r in ((False, False), (True, False), (False, True))}
ALL_PLANES_INST = {(nc, ks, m, f, r) for nc in (1, 2) for ks in (1, 2, 4) for m in (0, 1)
                   for f, r in ((False, False), (True, False), (False, True))}


def silu_trips(d):
    """Trips of silu_and_mul_kernel's column loop for the thread with the most work."""
    per_trip = min(-(-d // ROW), SILU_MAX_CHUNKS) * ROW
    return -(-d // per_trip)


def resadd_trips(numel):
    n8 = numel // CHUNK
    per_trip = min(-(-n8 // TPB), RESADD_MAX_BLOCKS) * TPB
    return -(-n8 // per_trip)


# ---- widths -------------------------------------------------------------------------------------------------------------------------
def _edges(bounds, last):
    """8, every boundary and the width one chunk past it, and the widest row."""
    return tuple(sorted({CHUNK, last} | {b + o for b in bounds for o in (0, CHUNK) if b + o <= last}))


# qs_invoke_quant, qs_silu_and_mul_quant: 512 | 520 = the block sum gains a second, one-chunk block; 2048 = TPB * 8 (NC 1 -> 2 at 256
# threads); 4096 = WIDE_ROW (256 -> 1024 threads); 8192 = 1024 * 8 and 16 384 (NC 1 -> 2 -> 4 at 1024 threads); 32 768 = the limit
QUANT_WIDTHS = _edges((BLOCK, ROW, WIDE_ROW, WIDE_NT * CHUNK, 2 * WIDE_NT * CHUNK), QUANT_MAX)
# qs_rms_norm_general, qs_add_residual_rms_norm_general: NC = 1, 2, 4, 4, 8 by ceil(H / 2048); FULL at H = NC * 2048.  6144: NC = 4 with
# exactly three chunks per thread and FULL off (every thread's fourth chunk is empty); 6152 adds a one-thread fourth chunk; 16 384 = limit
NORM_WIDTHS = _edges((ROW, 2 * ROW, 3 * ROW, 4 * ROW), NORM_MAX)
# qs_add_residual_rms_norm_general_planes: NC = 1 | 2 at 2048, FULL at 2048 and 4096 (= the limit); one chunk either side of both, and a
# half-filled last chunk set (1024, 3072)
PLANES_WIDTHS = tuple(sorted({CHUNK, ROW // 2, ROW - CHUNK, ROW, ROW + CHUNK, ROW + ROW // 2, PLANES_MAX - CHUNK, PLANES_MAX}))
PLANES_KS = (1, 2, 4)
PLANES_MODES = ("per_channel", "per_channel_fma", "per_group")     # epilogue convention 0 / 1 (common.h epi_per_chn) / per-group
# qs_rms_norm: a loop of TPB * 8 columns per trip - one full trip, one chunk into the second, the third and the ninth
RMS_WIDTHS = (CHUNK, ROW, ROW + CHUNK, 2 * ROW + CHUNK, 8 * ROW + CHUNK)
# qs_silu_and_mul: grid.y = min(ceil(d / 2048), 16) - one trip up to 32 768 columns; one chunk and a whole trip beyond
SILU_WIDTHS = (CHUNK, ROW, SILU_MAX_CHUNKS * ROW, SILU_MAX_CHUNKS * ROW + CHUNK, 2 * SILU_MAX_CHUNKS * ROW)
# qs_residual_add: min(ceil(numel / 8 / 256), 2048) workgroups - one trip up to 4 194 304 values; one chunk beyond; three trips and a bit
_RA = RESADD_MAX_BLOCKS * ROW
RESADD_SIZES = (CHUNK, _RA, _RA + CHUNK, 3 * _RA + 3 * CHUNK)


# ---- rows ---------------------------------------------------------------------------------------------------------------------------
Batch = collections.namedtuple("Batch", "family rows gamma pair notes bad_row")
Batch.__doc__ = """One launch.  rows: fp16 [T, H], the row the quantiser / norm sees (for the add entries the SUM, for the silu entries the
product).  gamma: fp16 [H] or None (the default gamma).  pair: None, or explicit (a, b) operands - (hidden, delta) for the add entries,
(gate, up) for the silu entries - where `rows` cannot be split (overflow in the add / in the product); rows is then None.
notes: one dict per row.  bad_row: index of the overflow row sandwiched between the two ordinary rows, or None."""


def _rng(h, seed):
    return np.random.default_rng(1000003 * seed + h)


def default_gamma(h):
    return _rng(h, 77).uniform(0.5, 1.5, h).astype(np.float16)


def ordinary_rows(h):
    """The two ordinary rows of every sandwich (and, run alone with the first repeated, their own reference)."""
    return (_rng(h, 5).standard_normal((2, h)) * 1.5 + 0.3).astype(np.float16)


def planted_positions(h, nt):
    """0, 7, 8 (the first chunk's ends and the second chunk's start), the last element of the first 512-block, the first element of every
    chunk set c * nt * 8 that exists at this width, H - 8 and H - 1 (the last chunk: partial chunk set wherever H % (nt * 8) != 0)."""
    pos = {0, 7, h - 8, h - 1}
    pos |= {p for p in (8, BLOCK - 1) if p < h}
    pos |= {c * nt * CHUNK for c in range(-(-h // (nt * CHUNK)))}
    return sorted(pos)


def _pos_note(p, h, nt):
    cs = nt * CHUNK
    last = (h - 1) // cs
    return dict(pos=p, chunk_set=p // cs, last_chunk=p >= h - CHUNK, partial_set=bool(h % cs) and p // cs == last)


def _split(rows, notes, family, gamma=None):
    """Batches of at most 8 rows; a tail shorter than 3 rows is filled up with ordinary rows."""
    out = []
    for i in range(0, len(rows), 8):
        r, n = rows[i:i + 8], list(notes[i:i + 8])
        if len(r) < 3:
            k = 3 - len(r)
            r = np.concatenate([r, ordinary_rows(rows.shape[1])[np.arange(k) % 2]])
            n += [dict(fill=True)] * k
        out.append(Batch(family, np.ascontiguousarray(r), gamma, None, n, None))
    return out


def planted(h, nt, seed=1):
    """Small background (N(0, 0.05)), |x[p]| = 3 the row's maximum: two rows per position, +3 and -3."""
    pos = [p for p in planted_positions(h, nt) for _ in (0, 1)]
    rows = (_rng(h, seed).standard_normal((len(pos), h)) * 0.05).astype(np.float16)
    for i, p in enumerate(pos):
        rows[i, p] = 3.0 if i % 2 == 0 else -3.0
    return _split(rows, [_pos_note(p, h, nt) for p in pos], "planted")


def one_hot(h, nt):
    """The same positions and signs (-1.5 first), the rest of the row +0.0."""
    pos = [p for p in planted_positions(h, nt) for _ in (0, 1)]
    rows = np.zeros((len(pos), h), np.float16)
    for i, p in enumerate(pos):
        rows[i, p] = -1.5 if i % 2 == 0 else 1.5
    return _split(rows, [_pos_note(p, h, nt) for p in pos], "one_hot")


TIE_VALUES = np.arange(-127, 127, dtype=np.float32) + np.float32(0.5)      # k + 0.5, k = -127 .. 126: all exact in fp16


def ties(h):
    """amax = 127 exactly (elements 0 / 1 = +127 / -127, which must quantise to +-127, never -128), so 127 / amax = 1 and every other
    element k + 0.5 is an exact rounding tie in fp32: the quantiser must round to even.  Three rows walk through the 254 tie values from
    different offsets; notes[r]["tie"] marks the tie elements (all but the first two)."""
    rows = np.empty((3, h), np.float16)
    for r in range(3):
        rows[r] = TIE_VALUES[(np.arange(h) + r * 85) % TIE_VALUES.size]
        rows[r, 0], rows[r, 1] = 127.0, -127.0
    mask = np.ones(h, bool)
    mask[:2] = False
    return [Batch("ties", rows, None, None, [dict(tie=mask)] * 3, None)]


def outlier(h, seed=2):
    """One channel of 65 504 (fp16 max) over N(0, 1): at the start, in the middle chunk, at the very end."""
    rows = _rng(h, seed).standard_normal((3, h)).astype(np.float16)
    pos = (0, (h // 2) // CHUNK * CHUNK, h - 1)
    for r, p in enumerate(pos):
        rows[r, p] = 65504.0 if r != 1 else -65504.0
    return [Batch("outlier", rows, None, None, [dict(pos=p) for p in pos], None)]


def _sandwich(family, bad, note, gamma=None):
    o = ordinary_rows(bad.shape[0])
    return Batch(family, np.stack([o[0], bad, o[1]]), gamma, None, [dict(ordinary=0), note, dict(ordinary=1)], 1)


def overflow(h, seed=3):
    """Rows holding +inf, -inf, a NaN (in the last chunk / in the first / in the chunk of the row's maximum, so that a thread whose
    chain a NaN poisons would lose the maximum), nothing but NaN, and both infinities - each between the two ordinary rows, which
    must come out exactly as when they run alone."""
    base = _rng(h, seed).standard_normal(h).astype(np.float16)
    out = []
    for name, edits in (("pos_inf_last", {h - 1: np.inf}), ("neg_inf_first", {0: -np.inf}), ("nan_last", {h - 1: np.nan}),
                        ("nan_first", {0: np.nan}), ("nan_by_max", {h - 1: np.nan, h - 2: -9.0}),
                        ("both_inf", {0: np.inf, h - 1: -np.inf})):
        bad = base.copy()
        for p, v in edits.items():
            bad[p] = v
        out.append(_sandwich("overflow", bad, dict(kind=name)))
    out.append(_sandwich("overflow", np.full(h, np.nan, np.float16), dict(kind="all_nan")))
    return out


def alone(h):
    """The ordinary rows without a bad row between them (the reference of every sandwich): [o0, o0, o1]."""
    o = ordinary_rows(h)
    return Batch("alone", np.stack([o[0], o[0], o[1]]), None, None, [dict(ordinary=0), dict(ordinary=0), dict(ordinary=1)], None)


def subnormal(h, seed=4):
    """Row 0: every element an fp16 subnormal (k * 2^-24, k = 1 .. 1023, either sign); row 1: subnormals mixed with -0.0; row 2: nothing
    but -0.0."""
    r = _rng(h, seed)
    k = r.integers(1, 1024, (2, h)).astype(np.uint16) | (r.integers(0, 2, (2, h)).astype(np.uint16) << 15)
    rows = np.empty((3, h), np.float16)
    rows[:2] = k.view(np.float16)
    rows[1, r.random(h) < 0.5] = -0.0
    rows[2] = -0.0
    return [Batch("subnormal", rows, None, None, [dict(kind="subnormal"), dict(kind="subnormal_negzero"), dict(kind="negzero")], None)]


def flat(h, seed=6):
    """Norm entries only.  Row 0: the constant 4.0 - H * 4 and its quotient by H are exact, the variance is 0, every normalised value 0:
    amax stays half(1e-6), scale = half(half(1e-6) / 127) = 0, an all-zero int8 row.  Row 1: the constant 0.1, whose fp32 sum chain
    rounds and leaves a tiny residue.  Row 2: 1000 + k / 2, k in -2 .. 2: the mean three orders above the spread.  Row 3: -0.25."""
    rows = np.empty((4, h), np.float16)
    rows[0], rows[1], rows[3] = 4.0, 0.1, -0.25
    rows[2] = 1000.0 + _rng(h, seed).integers(-2, 3, h) * 0.5
    return [Batch("flat", rows, None, None, [dict(kind=k) for k in ("const4", "const0.1", "mean1000", "const-0.25")], None)]


def gammas(h, seed=8):
    """Norm entries only: ordinary rows under a gamma holding zeros and negative values, a gamma of 65 504 throughout (the normalised
    fp16 value overflows to inf: amax = scale = inf, an all-zero int8 row), and a gamma of 0 throughout."""
    r = _rng(h, seed)
    rows = (r.standard_normal((3, h)) * 1.5 + 0.3).astype(np.float16)
    mixed = r.uniform(-1.5, 1.5, h).astype(np.float16)
    mixed[r.random(h) < 0.25] = 0.0
    mixed[h - 1] = -2.0
    out = []
    for name, g in (("mixed", mixed), ("huge", np.full(h, 65504.0, np.float16)), ("zero", np.zeros(h, np.float16))):
        out.append(Batch("gamma", rows, g, None, [dict(gamma=name)] * 3, None))
    return out


def quant_batches(h):
    """Everything qs_invoke_quant(_fuse_sum) runs at width h."""
    nt = quant_inst(h)[1]
    return planted(h, nt) + one_hot(h, nt) + ties(h) + outlier(h) + overflow(h) + [alone(h)] + subnormal(h)


def norm_batches(h):
    """Everything the norm entries run at width h (256 threads whatever the width)."""
    return planted(h, TPB) + one_hot(h, TPB) + ties(h) + outlier(h) + overflow(h) + [alone(h)] + subnormal(h) + flat(h) + gammas(h)


def split_for_add(rows):
    """(hidden, delta) whose fp16 sum is close to `rows` and keeps its structure: 3/4 and 1/4 of every element (zeros keep their sign,
    inf and NaN stay)."""
    f = rows.astype(np.float32)
    with np.errstate(invalid="ignore"):
        return (f * np.float32(0.75)).astype(np.float16), (f * np.float32(0.25)).astype(np.float16)


def add_overflow(h, seed=9):
    """Add entries only: 60 000 + 60 000 = +inf and -60 000 + -60 000 = -inf in the residual add (neither operand is inf)."""
    base = _rng(h, seed).standard_normal(h).astype(np.float16)
    out = []
    for name, p, v in (("pair_pos_last", h - 1, 60000.0), ("pair_neg_first", 0, -60000.0)):
        a, b = split_for_add(np.stack([ordinary_rows(h)[0], base, ordinary_rows(h)[1]]))
        a[1, p] = b[1, p] = v
        out.append(Batch("add_overflow", None, None, (a, b), [dict(ordinary=0), dict(kind=name), dict(ordinary=1)], 1))
    return out


def add_norm_batches(h):
    return norm_batches(h) + add_overflow(h)


SILU_GATE = 32.0     # >= 18: 1 + exp2(-32 log2 e) is 1.0 in fp32, silu(32) = 32 exactly - the product does not depend on `exp`


def split_for_silu(rows):
    """(gate, up) whose product is the row up to one fp16 rounding of row / 32: gate = 32, up = half(row / 32)."""
    with np.errstate(invalid="ignore"):
        up = (rows.astype(np.float32) / np.float32(SILU_GATE)).astype(np.float16)
    return np.full_like(up, SILU_GATE), up


def silu_overflow(d):
    """gate = up = 300: silu(300) = 300, the product 90 000 is +inf in fp16 - in the last chunk, between the ordinary rows."""
    g, u = split_for_silu(np.stack([ordinary_rows(d)[0], ordinary_rows(d)[0], ordinary_rows(d)[1]]))
    g[1, d - 1] = u[1, d - 1] = 300.0
    return [Batch("silu_overflow", None, None, (g, u), [dict(ordinary=0), dict(kind="300x300"), dict(ordinary=1)], 1)]


def silu_quant_batches(d):
    return quant_batches(d) + silu_overflow(d)


# silu regions: (gate, region).  ge18: 1 + exp2(-x log2 e) rounds to 1.0 (exp2 < 2^-24 from x = 16.7 on), silu(x) = x * rcp(1.0) = x.
# le-104: exp2(150) = inf, rcp = 0, x * 0 = -0.  Subnormal gates k * 2^-24 with k EVEN: silu(x) = x / 2 * (1 + x / 2 ...) - x / 2 is on
# the fp16 subnormal grid and the relative excess x / 2 <= 3e-5 is far from the next rounding boundary, so a last-place difference in
# exp2 or rcp cannot move the fp16 result (for odd k, x / 2 is an exact tie of that grid and the result hangs on the last bit of exp).
_SUB = np.float32(2.0 ** -24)
SILU_GATES = ([(v, "ge18") for v in (18.0, 20.0, 32.0, 100.0, 1000.0, 65504.0)] +
              [(v, "le-104") for v in (-104.0, -128.0, -1000.0, -65504.0)] +
              [(s * k * _SUB, "subnormal") for k in (2, 4, 10, 512, 1022) for s in (1.0, -1.0)] +
              [(np.inf, "inf"), (-np.inf, "inf"), (np.nan, "nan")])
SILU_UPS = (1.0, -1.0, 300.0, float(3 * _SUB))


def silu_regions(d):
    """fp16 [3, 2 d]: every (gate, up) of SILU_GATES x SILU_UPS, walked through cyclically from a different offset in every row."""
    pairs = [(g, u) for g, _ in SILU_GATES for u in SILU_UPS]
    gate = np.array([p[0] for p in pairs], np.float32)
    up = np.array([p[1] for p in pairs], np.float32)
    x = np.empty((3, 2 * d), np.float16)
    for r in range(3):
        idx = (np.arange(d) + 29 * r) % len(pairs)
        x[r, :d], x[r, d:] = gate[idx], up[idx]
    return x


def rms_exact_rows(h, seed=10):
    """rms_norm rows whose sum of squares is exact in any order: |x| = 2 everywhere, signs mixed (mean square exactly 4)."""
    return np.where(_rng(h, seed).random((3, h)) < 0.5, -2.0, 2.0).astype(np.float16)


def gaussian(t, h, seed, scale=1.0):
    return (_rng(h, seed).standard_normal((t, h)) * scale).astype(np.float16)


# ---- planes -------------------------------------------------------------------------------------------------------------------------
PLANES_K = 4096
ACC_MAX = 127 * 15 * PLANES_K       # the largest |accumulator| a per-channel K = 4096 GEMM can reach (int8 x uint4)
BIG = 1 << 30


def planes_problem(t, h, ks, family, seed=11):
    """int32 planes [ks, t, h] and their int32 sum `acc`.  `random`: typical accumulators (sigma = sqrt(K) * 340) with one row at
    +-ACC_MAX, cut into ks planes at random.  `cancel` (ks >= 2): plane 0 = acc + 2^30, plane 1 = -2^30 (ks = 4: planes 2, 3 the same
    again with acc's share split): summed as integers they give acc, converted to fp32 first they lose acc's low 7 bits."""
    r = _rng(h, seed + ks)
    acc = np.rint(r.standard_normal((t, h)) * (PLANES_K ** 0.5 * 340)).astype(np.int64)
    acc[t - 1] = np.where(r.random(h) < 0.5, -ACC_MAX, ACC_MAX)
    acc[0, ::2] |= 1                                                 # odd: the low bits are there to be lost
    planes = np.zeros((ks, t, h), np.int64)
    if family == "random":
        for z in range(ks - 1):
            planes[z] = r.integers(-ACC_MAX, ACC_MAX + 1, (t, h))
        planes[ks - 1] = acc - planes[:ks - 1].sum(axis=0)
    else:
        assert family == "cancel" and ks >= 2
        share = acc // 2 if ks == 4 else acc
        planes[0], planes[1] = share + BIG, -BIG
        if ks == 4:
            planes[2], planes[3] = -BIG, (acc - share) + BIG
    assert np.abs(planes).max() < 2 ** 31
    return planes.astype(np.int32), acc.astype(np.int32)


def planes_operands(t, h, seed=12):
    """The GEMM's epilogue operands (the ranges of oracle.synth) and the residual side: wscales, w_szs [h]; ascales, a_ssums [t];
    hidden [t, h]; gamma [h]."""
    r = _rng(h, seed)
    ws = r.uniform(0.002, 0.02, h).astype(np.float16)
    wz = (ws.astype(np.float32) * r.integers(0, 16, h)).astype(np.float16)
    sa = r.uniform(0.005, 0.05, t).astype(np.float16)
    ss = (r.standard_normal(t) * 20).astype(np.float16)
    hidden = (r.standard_normal((t, h)) * 0.7).astype(np.float16)
    return dict(wscales=ws, w_szs=wz, ascales=sa, a_ssums=ss, hidden=hidden, gamma=default_gamma(h))


def planes_cases():
    """(hidden, k_slices, mode, refsum, family) of every planes launch."""
    return [(h, ks, m, ref, fam) for h in PLANES_WIDTHS for ks in PLANES_KS for m in PLANES_MODES for ref in (False, True)
            for fam in (("random", "cancel") if ks > 1 else ("random",))]
