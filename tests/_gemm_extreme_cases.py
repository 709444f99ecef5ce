"""Extreme, structured operands for every W4A8 / W8A8 GEMM family: builders and ONE table.  Pure numpy (no torch, no GPU).
tests/test_gemm_extremes_cpu.py proves on the CPU that every row is what it claims (accumulators beyond 2^24 that fp32 cannot hold,
slices that cancel, the inf / NaN layout of the overflow scales, the plan the row is meant to run under);
tests/test_gemm_extremes_gpu.py runs the rows.  The complement of oracle.synth: its uniform random problems never contain -128 and keep
|acc| near sqrt(K) * 340, three orders of magnitude below 2^24 - where an int32 sum, a per-slice conversion followed by an fp32 sum, a
truncating and a rounding conversion are all the same number.

Activations A [M, K]: row i carries pattern PATTERNS[i % 7] (one launch carries all of them; M = 1 carries `odd`)
    odd            127 everywhere, element 0 = 126: against a weight of 15 or 127 the accumulator is 1 mod 4 - not a multiple of the
                   fp32 spacing at its magnitude (2 in [2^24, 2^25), 4 in [2^25, 2^26), 8 at 2^26); (float)acc rounds it TOWARDS
                   zero, as truncation would
    odd3           elements 0 .. 2 = 126: 3 mod 4, so (float)acc rounds it AWAY from zero - where a truncating conversion differs
    neg128 pos127  every element -128 / 127
    cancel_halves  +127 on k < K/2, -128 on the rest
    cancel_k128    the sign flips every 128 elements (the k-step of every kernel): the waves of a split-K workgroup and the K-groups of
                   a ring workgroup take k-steps round-robin, so each holds a large same-sign partial
    checker        the sign flips every element
Weights (`wkind`), every one with columns of one sign and value throughout
    per-channel    q15: q = 15 everywhere; q15_half: odd channels have q = 0 on the second half of K.  z = channel mod 16, so w_sz = 0
                   occurs; s1 = 0.01
    bytes          b127 / bm128: every dequantised byte 127 / -128; mixed: channels 0, 1 mod 4 are 127 / -128 throughout, channels 2, 3
                   mod 4 alternate between the two per 128-group.  per_group: (q, z, s2) = (2, 1, 127) and (0, 1, 128) through
                   w4a8.pack_per_group, inside the protective range; per_group_any_bytes: q = 15 with raw level-2 bytes S = 17 and
                   Z = 128 / 129 (15 * 17 + Z wraps to 127 / -128; no (z, s2) pair gives those bytes); w8a8: the bytes themselves
Scales: ascales = 0.03 (`finite`: |a_ssums| <= 55 040 at K = 14 336) or 0.05 (`overflow`: the same-sign rows at K = 14 336 have
a_ssums = +-inf, so the columns with w_sz = 0 are NaN and the others +-inf); a_ssums = half(ascale * sum A), as the quantiser forms it.

K: the smallest multiple of 128 at which 127 * 15 * K (8832) or 127 * 127 * K (1152) reaches 2^24, and a project K above it (14 336,
2176).  Where a geometry does not divide those, the row takes the smallest K above that fits and its note says so.  Partials that cancel:
with |a w| <= 128 * 15 the halves of a per-channel row stay below 2^24 up to K = 17 476, beyond this table's sizes - such rows claim
2^23; byte rows reach 2^24 per half from K = 2081 on, and every family has such a row (CPU test)."""
import collections
import functools

import numpy as np

from oracle import w4a8

T24 = 1 << 24
PATTERNS = ("odd", "neg128", "cancel_halves", "pos127", "cancel_k128", "checker", "odd3")
SAME_SIGN = ("odd", "neg128", "pos127", "odd3")
MODES = ("per_channel", "per_group", "per_group_any_bytes")
ASCALE = {"finite": 0.03, "overflow": 0.05}
S1 = 0.01


# ---- operands -----------------------------------------------------------------------------------------------------------------------------
def pattern_row(name, K):
    k = np.arange(K)
    if name == "neg128":
        return np.full(K, -128, np.int8)
    if name in ("pos127", "odd", "odd3"):
        row = np.full(K, 127, np.int8)
        row[:{"pos127": 0, "odd": 1, "odd3": 3}[name]] = 126
        return row
    flip = {"cancel_halves": k >= K // 2, "cancel_k128": (k // 128) % 2 == 1, "checker": k % 2 == 1}[name]
    return np.where(flip, -128, 127).astype(np.int8)


def row_patterns(M):
    """The pattern of each of the M rows."""
    return [PATTERNS[i % len(PATTERNS)] for i in range(M)]


def activations(M, K):
    return np.stack([pattern_row(p, K) for p in PATTERNS])[np.arange(M) % len(PATTERNS)]


def _bytes(N, K, wkind):
    """The dequantised int8 weights [N, K] of a byte kind."""
    if wkind in ("b127", "bm128"):
        return np.full((N, K), 127 if wkind == "b127" else -128, np.int8)
    assert wkind == "mixed"
    n, g = np.arange(N)[:, None], (np.arange(K) // 128)[None, :]
    neg = np.where(n % 4 < 2, n % 4 == 1, (g + n) % 2 == 1)
    return np.where(neg, -128, 127).astype(np.int8)


@functools.lru_cache(maxsize=None)
def weights(mode, N, K, wkind):
    """-> dict: the entry's weight operands, `W` = the integers [N, K] the accumulator multiplies (nibbles 0 .. 15 per-channel, the
    dequantised bytes otherwise), and per-channel `z`."""
    s1 = np.full(N, S1, np.float16)
    if mode == "per_channel":
        q = np.full((N, K), 15, np.uint8)
        if wkind == "q15_half":
            q[1::2, K // 2:] = 0
        else:
            assert wkind == "q15"
        z = (np.arange(N) % 16).astype(np.uint8)
        qweight, wscales, w_szs = w4a8.pack_per_channel(q, z, s1)
        return dict(W=q, z=z, qweight=qweight, wscales=wscales, w_szs=w_szs)
    W = _bytes(N, K, wkind)
    if mode == "w8a8":
        return dict(W=W, weight=W, wscales=s1)
    neg = W[:, ::128] < 0                                               # [N, K/128]: the group's byte is -128
    if mode == "per_group":
        q = np.repeat(np.where(neg, 0, 2), 128, axis=1)
        qweight, wscales, s2_scales, s2_zeros = w4a8.pack_per_group(q, np.ones_like(neg, np.int32), np.where(neg, 128, 127), s1)
    else:
        assert mode == "per_group_any_bytes"
        qweight, wscales = w4a8.pack_qweight(np.full((N, K), 15, np.uint8)), s1
        s2_scales = w4a8.permute_group_meta(np.full(neg.T.shape, 17, np.uint8)).view(np.int8)
        s2_zeros = w4a8.permute_group_meta(np.where(neg.T, 129, 128).astype(np.uint8)).view(np.int8)
    assert np.array_equal(w4a8.dequant_per_group_w8(qweight, s2_zeros, s2_scales), W), "the packed bytes are not the intended ones"
    return dict(W=W, qweight=qweight, wscales=wscales, s2_scales=s2_scales, s2_zeros=s2_zeros)


@functools.lru_cache(maxsize=None)
def problem(mode, M, N, K, wkind, scales="finite"):
    """One problem per key, shared by every row and test that uses it; nothing writes to it."""
    pr = dict(weights(mode, N, K, wkind), A=activations(M, K), mode=mode)
    if scales == "tie":
        sa, pr["wscales"] = tie_scales(mode, N, K, wkind)
        pr["ascales"] = np.full(M, sa, np.float16)
        if mode == "per_channel":
            pr["w_szs"] = (pr["z"].astype(np.float16) * pr["wscales"]).astype(np.float16)        # as w4a8.pack_per_channel
    else:
        pr["ascales"] = np.full(M, ASCALE[scales], np.float16)
    if mode == "per_channel":
        with np.errstate(over="ignore"):                                # (the overflow set is meant to)
            pr["a_ssums"] = (pr["ascales"].astype(np.float32) * pr["A"].astype(np.int64).sum(axis=1).astype(np.float32)).astype(np.float16)
    return pr


@functools.lru_cache(maxsize=None)
def problem_acc(mode, M, N, K, wkind):
    """exact_acc of a problem (the scales do not enter), computed once."""
    pr = problem(mode, M, N, K, wkind)
    return exact_acc(pr["A"], pr["W"])


def exact_acc(A, W):
    """A.astype(int64) @ W.astype(int64).T.  A row of the product depends on that row of A alone, so where the rows of A repeat
    with the period of PATTERNS (checked here) the int64 product (no BLAS) is taken over the first period."""
    period = np.arange(A.shape[0]) % len(PATTERNS)
    if A.shape[0] > len(PATTERNS) and np.array_equal(A, A[:len(PATTERNS)][period]):
        return (A[:len(PATTERNS)].astype(np.int64) @ W.astype(np.int64).T)[period]
    return A.astype(np.int64) @ W.astype(np.int64).T


def oracle_acc(pr):
    """The oracle's int32 accumulators (int_matmul's sliced BLAS)."""
    if pr["mode"] == "per_channel":
        return w4a8.gemm_per_chn_acc(pr["A"], pr["qweight"])
    if pr["mode"] == "w8a8":
        return w4a8.gemm_w8a8(pr["A"], pr["weight"], pr["wscales"], pr["ascales"])[0]
    return w4a8.gemm_per_group_acc(pr["A"], pr["qweight"], pr["s2_zeros"], pr["s2_scales"])


def oracle_out(pr, acc, fma=False):
    """The oracle's fp16 output of these accumulators; inf and NaN as the fp32 epilogue yields them."""
    with np.errstate(invalid="ignore", over="ignore"):
        if pr["mode"] == "per_channel":
            return w4a8.epilogue_per_chn(acc, pr["wscales"], pr["ascales"], pr["w_szs"], pr["a_ssums"], fma=fma)
        return w4a8.epilogue_per_group(acc, pr["wscales"], pr["ascales"])


def other_fp32(acc):
    """float32 [like acc]: where fp32 cannot hold the integer, the neighbour on the OTHER side of it from (float)acc - what a
    conversion that rounds differently (truncation, half away from zero) would give; (float)acc itself elsewhere."""
    f = acc.astype(np.float32)
    back = f.astype(np.int64)
    toward = np.where(back > acc, -np.inf, np.inf).astype(np.float32)
    return np.where(back == acc, f, np.nextafter(f, toward)).astype(np.float32)


def _f16_between(lo, hi):
    """Every fp16 value in [lo, hi] (positive)."""
    return np.arange(np.float16(lo).view(np.uint16), np.float16(hi).view(np.uint16) + 1, dtype=np.uint16).view(np.float16)


@functools.lru_cache(maxsize=None)
def tie_scales(mode, N, K, wkind):
    """-> (ascale, wscales fp16 [N]): the `tie` scales.  With the constant scales of the other two sets the fp16 output is almost
    always the same number whether the epilogue converts an accumulator beyond 2^24 to its nearest fp32 neighbour or to the next one
    (the 11 significant bits of fp16 hide the 24th), so the fp16 comparisons there rarely see the rounding of (float)acc.  Here the scales
    are searched - ascale over fp16 values in [0.02, 0.035], wscale per channel over every fp16 value in [0.005, 0.02] - so that the
    product of an `odd` or `odd3` row lands next to an fp16 rounding boundary: with other_fp32(acc) in place of (float)acc the fp16
    output of that channel changes.  Channels 0 .. 31 mod 64 are searched for the `odd` row, the others for `odd3`; per-channel,
    channels 0 .. 15 mod 32 under the un-contracted epilogue and 16 .. 31 under the fmaf one.  Channels without a solution keep 0.01;
    tests/test_gemm_extremes_cpu.py holds every problem to at least one per row pattern and convention."""
    w = weights(mode, N, K, wkind)
    targets = np.stack([pattern_row("odd", K), pattern_row("odd3", K)])
    row = (np.arange(N) // 32) % 2                                        # the target row of a channel
    acc = exact_acc(targets, w["W"])[row, np.arange(N)]                   # its accumulator in that channel
    near, other = acc.astype(np.float32), other_fp32(acc)
    WS = _f16_between(0.005, 0.02)
    z = w["z"] if mode == "per_channel" else np.zeros(N, np.uint8)
    conv = (np.arange(N) // 16) % 2 if mode == "per_channel" else np.zeros(N, np.int64)
    classes = sorted({(int(a), int(zz), int(c)) for a, o, zz, c in zip(acc, near != other, z, conv) if o})
    assert classes, "no channel whose accumulator fp32 cannot hold"
    SA = _f16_between(0.02, 0.035)[::8]                                   # (a_ssums stays finite up to K = 14 336)
    sums = {int(a): int(s) for a, s in zip(acc, targets.astype(np.int64).sum(axis=1)[row])}   # sum A of the row an accumulator is of
    hits = {}
    for a, zz, c in classes:                                              # [ascale candidate, wscale candidate] per class
        sub = dict(mode=mode, wscales=WS, ascales=SA)
        if mode == "per_channel":
            sub["w_szs"] = (np.float16(zz) * WS).astype(np.float16)
            sub["a_ssums"] = (SA.astype(np.float32) * np.float32(sums[a])).astype(np.float16)
        values = np.int64(a).astype(np.float32), other_fp32(np.array([a], np.int64))[0]
        outs = [oracle_out(sub, np.full((SA.size, WS.size), v, np.float32), fma=bool(c)).view(np.uint16) for v in values]
        hits[(a, zz, c)] = outs[0] != outs[1]
    s = int(np.argmax(sum(h.any(axis=1).astype(np.int64) for h in hits.values())))
    found = {k: WS[np.flatnonzero(h[s])[0]] for k, h in hits.items() if h[s].any()}
    sa = SA[s]
    wscales = np.array([found.get((int(a), int(zz), int(c)), np.float16(S1)) for a, zz, c in zip(acc, z, conv)], np.float16)
    return np.float16(sa), wscales


def fp32_spacing(v):
    """Distance between neighbouring float32 values at the magnitude of the integers v (1 below 2^24)."""
    return np.maximum(1, 1 << np.maximum(0, np.floor(np.log2(np.maximum(np.abs(v), 1))).astype(np.int64) - 23))


# ---- the table ----------------------------------------------------------------------------------------------------------------------------
# family: own = the planner's choice; splitk / pair / tiled / wide / ring = forced by `code` (include/qserve_amd.h qs_gemm_variant_code);
# every row of these six also runs the raw-accumulator entry (gemm_forward_acc).  planes = the K-slice planes entries finished by
# add_residual_rms_norm_general_planes; gate_up = GEMM + silu * mul in one call; moe = the grouped GEMM; w8a8.
# plan: what the planner must report for the row - qs_w4a8_gemm_plan's (family, p0 .. p3), None = not pinned; planes:
# qs_w4a8_gemm_planes_plan's (k_slices, m_tiles, units, token blocks); moe: qs_moe_gemm_plan's (mt, waves, row blocks, units).
# extra: moe = rows per expert (M = their sum, over 14 source rows).
Row = collections.namedtuple("Row", "family code mode M N K wkind scales plan note extra")
F_SPLITK, F_PAIR, F_RING, F_TILED, F_WIDE = 1, 2, 3, 4, 5
PC, PG, ANY = MODES
PC_K, BYTE_K = (8832, 14336), (1152, 2176)


def _row(family, code, mode, M, N, K, wkind, scales="finite", plan=None, note="", extra=None):
    return Row(family, code, mode, M, N, K, wkind, scales, plan, note, extra)


def ring_geometry(code):
    """(m_tiles, units, k_slices) of a ring (41xx ..) or planes (46xx ..) code."""
    g = (code - 4100) % 500
    return g % 100 // 10, g % 10, g // 100 + 1


def ring_fits(code, N, K):
    """csrc/gemm_plan.h ring_fits, restated."""
    _, wn, ks = ring_geometry(code)
    return N % (64 * wn) == 0 and (K // 64) % ks == 0 and (K // 64 // ks) % (8 // wn) == 0


def ring_k(code, N, want):
    """The smallest multiple of 128 from `want` on that the geometry divides, and the note that says so."""
    K = next(k for k in range(want, 16384, 128) if ring_fits(code, N, k))
    return K, "" if K == want else f"K {want} -> {K}: the nearest the geometry divides"


OWN = [
    _row("own", -1, PC, 1, 64, 8832, "q15", plan=(F_SPLITK, 1, 8, 1, 0)),
    _row("own", -1, PC, 17, 192, 14336, "q15_half", plan=(F_RING, 1, 1, 2, 4)),
    _row("own", -1, PC, 130, 512, 14336, "q15", "overflow", plan=(F_RING, 2, 1, 5, 4)),
    _row("own", -1, PC, 130, 512, 8832, "q15_half", plan=(F_RING, 4, 4, 3, 1)),
    _row("own", -1, PG, 1, 64, 1152, "b127", plan=(F_SPLITK, 1, 4, 1, 0)),
    _row("own", -1, PG, 17, 192, 2176, "mixed", plan=(F_SPLITK, 2, 8, 1, 0)),
    _row("own", -1, PG, 130, 512, 2176, "bm128", plan=(F_RING, 4, 4, 3, 1)),
    _row("own", -1, ANY, 17, 64, 2176, "mixed", plan=(F_SPLITK, 2, 8, 1, 0)),
    _row("own", -1, ANY, 130, 192, 1152, "b127", plan=(F_SPLITK, 4, 4, 1, 0)),
]

# one un-split and one cross-block row per wave count: (mo, S, NW, M, N, plan) of _gemm_family_cases.SPLITK, K replaced
_SPLITK = [(1, 1, 1, 1, 64, (1, 1, 1, 0)), (2, 3, 1, 64, 512, (2, 1, 3, 1)), (1, 1, 2, 33, 192, (1, 2, 1, 1)), (3, 2, 2, 50, 192, (3, 2, 2, 1)),
           (1, 1, 4, 65, 512, (1, 4, 1, 1)), (1, 4, 4, 130, 64, (1, 4, 4, 1)), (1, 1, 8, 16, 64, (1, 8, 1, 0)), (1, 2, 8, 17, 192, (1, 8, 2, 1))]


def _splitk_rows():
    rows = []
    for i, (mo, S, NW, M, N, plan) in enumerate(_SPLITK):
        for j, mode in enumerate(MODES):
            K = (PC_K if mode == PC else BYTE_K)[(i // 2 + j + 1) % 2]
            wkind = ("q15", "q15_half")[i % 2] if mode == PC else ("b127", "mixed", "bm128")[(i + j) % 3]
            if M == 1 and wkind == "bm128":                              # (a lone `odd` row needs a weight that is no power of two)
                wkind = "mixed"
            rows.append(_row("splitk", 1000 + 100 * mo + 10 * S + NW, mode, M, N, K, wkind,
                             "overflow" if mode == PC and K == 14336 and i % 2 == 1 else "finite", plan=(F_SPLITK,) + plan))
    return rows


SPLITK = _splitk_rows()

PAIR = [
    _row("pair", 2001, PC, 1, 512, 8832, "q15", plan=(F_PAIR, None, None, None, None)),
    _row("pair", 2001, PC, 17, 512, 14336, "q15_half", "overflow", plan=(F_PAIR, None, None, None, None)),
    _row("pair", 2001, PC, 130, 512, 14336, "q15", plan=(F_PAIR, None, None, None, None)),
    _row("pair", 2001, PG, 1, 512, 1152, "b127", plan=(F_PAIR, None, None, None, None)),
    _row("pair", 2001, PG, 17, 512, 2176, "mixed", plan=(F_PAIR, None, None, None, None)),
    _row("pair", 2001, PG, 130, 512, 2176, "bm128", plan=(F_PAIR, None, None, None, None)),
    _row("pair", 2001, ANY, 130, 512, 2176, "mixed", plan=(F_PAIR, None, None, None, None)),
]

# 3001 / 3003 force the eight- and the four-wave 256-token tile; each row runs with three workgroups walking the tiles and with one
# workgroup per tile (3220 / 3210), as tests/test_gemm_gpu.py::test_tiled_workgroup_walks_several_tiles
TILED = [_row(fam, code, mode, M, 512, K, wkind, scales, plan=(plan0, 8, None, None, None))
         for fam, code, plan0 in (("tiled", 3001, F_TILED), ("wide", 3003, F_WIDE))
         for mode, M, K, wkind, scales in ((PC, 130, 14336, "q15" if code == 3001 else "q15_half", "overflow"),
                                           (PC, 17, 8832, "q15_half" if code == 3001 else "q15", "finite"),
                                           (PG, 130, 2176, "mixed" if code == 3001 else "b127", "finite"),
                                           (PG, 17, 1152, "bm128" if code == 3001 else "mixed", "finite"))]

# one row per variant of RING and KXCD in tests/test_gemm_gpu.py, in every mode.  K-sliced rows (42xx, 44xx) run with the K slices
# across the XCDs and on one XCD (ring flag 4096), as test_k_slices_across_xcds_and_on_one_xcd_are_exact
_RING = [(4111, 17, 64), (4121, 130, 192), (4141, 130, 512), (4122, 17, 512), (4142, 130, 384), (4144, 130, 512), (4182, 130, 128),
         (4211, 1, 64), (4221, 130, 512), (4241, 130, 512), (4222, 17, 512), (4244, 130, 256), (4282, 130, 384), (4411, 17, 192),
         (4421, 17, 512), (4422, 130, 512), (4442, 130, 512), (4482, 130, 128)]


def _ring_rows():
    rows = []
    for i, (code, M, N) in enumerate(_RING):
        mt, wn, ks = ring_geometry(code)
        for j, mode in enumerate(MODES):
            K, note = ring_k(code, N, (PC_K if mode == PC else BYTE_K)[(i + j) % 2])
            wkind = ("q15", "q15_half")[i % 2] if mode == PC else ("b127", "mixed", "bm128")[(i + j) % 3]
            if M == 1 and wkind == "bm128":                              # (a lone `odd` row needs a weight that is no power of two)
                wkind = "mixed"
            rows.append(_row("ring", code, mode, M, N, K, wkind, "overflow" if mode == PC and K == 14336 and i % 4 == 1 else "finite",
                             plan=(F_RING, mt, wn, ((M + 15) // 16 + mt - 1) // mt, ks), note=note))
    return rows


RING = _ring_rows()


def _planes(code, mode, M, N, want, wkind, scales="finite", plan=None):
    K, note = (want, "") if code < 0 else ring_k(code, N, want)
    return _row("planes", code, mode, M, N, K, wkind, scales, plan, note)


PLANES = [
    _planes(-1, PC, 17, 512, 14336, "q15", "overflow", plan=(4, 1, 1, 2)),
    _planes(-1, PC, 130, 512, 8832, "q15_half", plan=(1, 4, 4, 3)),
    _planes(4600 + 100 + 20 + 1, PC, 130, 192, 14336, "q15", plan=(2, 2, 1, 5)),
    _planes(4600 + 300 + 40 + 1, PC, 17, 64, 14336, "q15_half", "overflow", plan=(4, 4, 1, 1)),
    _planes(-1, PG, 130, 512, 2176, "mixed", plan=(1, 4, 4, 3)),
    _planes(4600 + 100 + 20 + 1, PG, 17, 192, 2176, "b127", plan=(2, 2, 1, 1)),
    _planes(4600 + 300 + 40 + 1, PG, 130, 64, 2176, "bm128", plan=(4, 4, 1, 3)),
    _planes(4600 + 10 + 1, PG, 17, 64, 1152, "mixed", plan=(1, 1, 1, 2)),
]


def _gate_up(code, mode, M, want, wkind, scales="finite", plan=None):
    K, note = ring_k(code, 512, want) if 4100 <= code < 4500 else (want, "")
    return _row("gate_up", code, mode, M, 512, K, wkind, scales, plan, note)


# N = 512 stacks [gate | up].  4222: K-sliced, no activation epilogue - the call runs its two launches
GATE_UP = [
    _gate_up(4111, PC, 17, 14336, "q15_half", plan=(F_RING, 1, 1, 2, 1)),
    _gate_up(3001, PC, 130, 14336, "q15", "overflow", plan=(F_TILED, 8, None, None, None)),
    _gate_up(4222, PC, 17, 8832, "q15", plan=(F_RING, 2, 2, 1, 2)),
    _gate_up(-1, PC, 130, 8832, "q15_half", plan=(F_RING, 4, 4, 3, 1)),
    _gate_up(4144, PG, 130, 2176, "mixed", plan=(F_RING, 4, 4, 3, 1)),
    _gate_up(3003, PG, 130, 1152, "b127", plan=(F_WIDE, 8, None, None, None)),
    _gate_up(4182, PG, 130, 2176, "mixed", plan=(F_RING, 8, 2, 2, 1)),
    _gate_up(-1, PG, 17, 2176, "bm128", plan=(F_SPLITK, 1, 8, 1, 1)),
]

# two experts: expert 0 the row's wkind, expert 1 all-zero nibbles (its z, s1 - or s2 = 1 - as expert 0); 14 source rows (every pattern
# twice), row_src with repeats
MOE_X_ROWS = 14
MOE = [
    _row("moe", -1, PC, 33, 192, 14336, "q15", plan=(2, 8, 3, 3), extra=(20, 13)),
    _row("moe", -1, PC, 10, 64, 14336, "q15_half", "overflow", plan=(1, 8, 2, 1), extra=(7, 3)),
    _row("moe", -1, PC, 110, 512, 8832, "q15", plan=(4, 4, 3, 8), extra=(70, 40)),
    _row("moe", -1, PG, 33, 192, 2176, "mixed", plan=(2, 8, 3, 3), extra=(20, 13)),
    _row("moe", -1, PG, 10, 512, 1152, "b127", plan=(1, 4, 2, 8), extra=(7, 3)),
    _row("moe", -1, PG, 110, 64, 2176, "bm128", plan=(4, 4, 3, 1), extra=(70, 40)),
]

W8A8 = [
    _row("w8a8", -1, "w8a8", 1, 64, 1152, "b127"),
    _row("w8a8", -1, "w8a8", 17, 192, 2176, "mixed"),
    _row("w8a8", -1, "w8a8", 130, 512, 2176, "bm128"),
    _row("w8a8", -1, "w8a8", 17, 64, 1152, "mixed"),
    _row("w8a8", -1, "w8a8", 130, 208, 2176, "b127", note="N = 208: 13 waves, the last workgroup has idle ones"),
]

def _tie_rows(rows):
    """The first finite row of every (family, mode, K slices or cross-block split) whose weights are not -128 alone, again with the `tie` scales."""
    seen, out = set(), []
    for r in rows:
        key = (r.family, r.mode, r.plan[4] if r.family == "ring" else r.plan[3] > 1 if r.family == "splitk" else r.plan[0] if r.family == "planes" else 0)
        if key not in seen and r.scales == "finite" and r.wkind != "bm128":
            seen.add(key)
            out.append(r._replace(scales="tie"))
    return out


TABLE = OWN + SPLITK + PAIR + TILED + RING + PLANES + GATE_UP + MOE + W8A8
TABLE = TABLE + _tie_rows(TABLE)
FAMILIES = ("own", "splitk", "pair", "tiled", "wide", "ring", "planes", "gate_up", "moe", "w8a8")


def row_id(row):
    return f"{row.family}{'' if row.code < 0 else row.code}-{row.mode}-M{row.M}-N{row.N}-K{row.K}-{row.wkind}-{row.scales}"


def source_rows(row):
    """Activation rows of the row's problem: M, or the 14 source rows a grouped GEMM gathers from."""
    return MOE_X_ROWS if row.family == "moe" else row.M


def row_problem_key(row):
    """The arguments of `problem_acc` for the row's problem."""
    return row.mode, source_rows(row), row.N, row.K, row.wkind


def row_problem(row):
    return problem(*row_problem_key(row), row.scales)


def moe_zero_expert(pr):
    """Expert 1 of a grouped row: all-zero nibbles under expert 0's scales (per-group: s2 = 1, zero byte 0 - dequantised bytes 0)."""
    N, K = pr["W"].shape
    e = dict(pr, W=np.zeros((N, K), np.int8), qweight=w4a8.pack_qweight(np.zeros((N, K), np.uint8)))
    if pr["mode"] != "per_channel":
        e["s2_scales"], e["s2_zeros"] = np.ones_like(pr["s2_scales"]), np.zeros_like(pr["s2_zeros"])
    return e


def moe_routing(row):
    """(expert_offsets int32 [3], row_src int32 [P]): repeats, no order."""
    offsets = np.concatenate([[0], np.cumsum(row.extra)]).astype(np.int32)
    row_src = np.random.default_rng(row.M + row.N).integers(0, MOE_X_ROWS, size=row.M).astype(np.int32)
    return offsets, row_src
