// gemm_plan.h -- which W4A8 GEMM kernel serves a problem, and with what geometry.  Plain C++17: no HIP, no device access, no
// global state, no error reporting - a plan is a function of (mode, act, M, N, K, variant) alone, so the whole table can be
// printed and pinned on a machine without a GPU (tests/host/gemm_plan_table.cpp, tests/test_gemm_plan_table_cpu.py).
// gemm_w4a8.hip launches what these functions return; qs_w4a8_gemm_plan / qs_w4a8_gemm_planes_plan report it.
//
// Every constant below is measured (scripts/bench_gemm*.py): a change must come with new measurements and a
// re-recorded tests/golden/gemm_plan_table.json.
#pragma once
#include "../../include/qserve_amd.h"

namespace gemm_plan {

// What the dispatcher launches for a problem: family (the plan5[0] codes of qs_w4a8_gemm_plan) and its geometry.
enum { GEMM_INVALID = -1, GEMM_NONE = 0, GEMM_SPLITK = 1, GEMM_PAIR = 2, GEMM_RING = 3, GEMM_TILED = 4, GEMM_WIDE = 5 };
struct GemmPlan {
    int family;   // GEMM_NONE: `act` asked for, no kernel with the activation epilogue serves the shape;
                  // GEMM_INVALID: a forced ring geometry that does not fit (p = the geometry asked for: mt, wn, 0, ksplit)
    int p[4];     // ring: mt, wn, mblocks, ksplit; tiled / wide: m-tiles per wave (8 = 256-token tile, 4 = 128);
                  // split-K: MT, NW, S, xcd_map
};

// the shapes every W4A8 entry accepts (the caller words the error)
enum ShapeFault { SHAPE_OK = 0, SHAPE_BAD, SHAPE_N_NOT_64, SHAPE_K_NOT_128 };
inline ShapeFault check_shape(int M, int N, int K) {
    return !(M >= 0 && N > 0 && K > 0) ? SHAPE_BAD : N % 64 != 0 ? SHAPE_N_NOT_64 : K % 128 != 0 ? SHAPE_K_NOT_128 : SHAPE_OK;
}
// the LDS-DMA kernels (ring, tiled, wide) address both operands with 32-bit offsets
inline bool offsets_fit(int M, int N, int K) {
    return (size_t)M * K < (1ull << 32) && (size_t)N * K / 2 < (1ull << 32);
}

// ---- the selection hook, decoded (include/qserve_amd.h qs_gemm_variant_code; `Variant d{code}`) ---------------------------------
// The production value of every field is the one QS_GEMM_DEFAULT gives; the rules below read these fields, never the codes.
struct Variant {
    int v;
    int tile_forced = v == QS_GEMM_TILED_256 || v == QS_GEMM_WIDE_256 ? 8 : v == QS_GEMM_TILED_128 ? 4 : 0;   // m-tiles per wave of a forced compute-bound tile
    bool tile_rule = v < QS_GEMM_SPLITK_BASE || v > QS_GEMM_WIDE_256;   // the measured crossovers choose the tile (3000 and every other code up to 3003: no)
    bool wide_forced = v == QS_GEMM_WIDE_256;     // the four-wave 256-token tile, per-channel too
    bool wide_barred = v == QS_GEMM_TILED_256;    // the eight-wave one, per-group too
    bool ring_forced = v >= QS_GEMM_RING_GEOMETRY_BASE && v < QS_GEMM_RING_GEOMETRY_END;   // + 100 * (ks - 1) + 10 * mt + wn (tests)
    int ring_ks = (v - QS_GEMM_RING_GEOMETRY_BASE) / 100 + 1, ring_mt = (v - QS_GEMM_RING_GEOMETRY_BASE) % 100 / 10, ring_wn = (v - QS_GEMM_RING_GEOMETRY_BASE) % 10;
    bool ring_rule = v != QS_GEMM_RING_OFF && (v < QS_GEMM_SPLITK_BASE || v >= QS_GEMM_RING_OFF);   // the byte model chooses a ring geometry ...
    bool k_slices = v != QS_GEMM_RING_NO_KSLICES;            // ... with K slices,
    bool group_term = v != QS_GEMM_RING_NO_GROUP_TERM;       // ... the per-group term,
    bool down_override = v != QS_GEMM_RING_NO_DOWN_OVERRIDE; // ... the measured override for Llama-3's down_proj
    bool mt8 = v != QS_GEMM_RING_NO_MT8;                     // ... and the 128-token geometry <8,2>
    bool pair_barred = v == QS_GEMM_PAIR_OFF, pair_forced = v == QS_GEMM_PAIR_FORCED;
    int splitk_code = v >= QS_GEMM_SPLITK_BASE && v < QS_GEMM_PAIR_OFF ? v - QS_GEMM_SPLITK_BASE : -1;   // 100 * mtile_override + 10 * S + NW, -1 = the kernel's own rule
    int planes_forced = v >= QS_GEMM_PLANES_GEOMETRY_BASE && v < QS_GEMM_PLANES_GEOMETRY_END ? v - QS_GEMM_PLANES_GEOMETRY_BASE : -1;   // as ring_forced, for the planes; -1 = any
};

// ---- the ring kernel's byte model: one table, one fit predicate, one cost ---------------------------------------------------
// A workgroup of (16 mt tokens) x (64 wn channels) streams K (16 mt + 32 wn) bytes through its CU, one workgroup per CU at a
// time, and the per-CU fill rate (~47 GB/s) is what bounds the decode shapes - so a search takes the geometry with the fewest
// bytes per CU over all its rounds (measured: scripts/bench_gemm.py, scripts/bench_gemm_shard.py for tensor-parallel shards).
//
// The geometries <mt, wn> the ring kernel is built for.  The ORDER is behaviour: ties go to the earlier entry - the two-unit
// workgroups (the activation tile is shared by two waves).  <4,4> = 4 units (2 K-groups): fewer bytes per CU where two-unit
// workgroups need a second round - M = 128 x N = 28 672: 26.8 vs 32.4 us (per-group 41.0 vs 47.0), M = 64 x 49 152: 48.9 vs 58.4.
struct RingGeo { int mt, wn; };
constexpr RingGeo RING_GEO[7] = {{4, 2}, {2, 2}, {4, 1}, {2, 1}, {1, 1}, {4, 4}, {8, 2}};
inline bool ring_geometry_exists(int mt, int wn) {
    for (const RingGeo& g : RING_GEO)
        if (g.mt == mt && g.wn == wn) return true;
    return false;
}
// channels divide into the workgroups' units; the 64-wide k-stages divide into ks slices and a slice's stages into the 8 / wn K-groups
inline bool ring_fits(int /*mt*/, int wn, int ks, int N, int K) {
    return N % (64 * wn) == 0 && (K / 64) % ks == 0 && (K / 64 / ks) % (8 / wn) == 0;
}
// bytes through the busiest CU: `blocks` workgroups over 256 CUs, each streaming `bytes_per_k` for every k of its `k` long
// stream, times tenths / 10 (what the kernel's overheads were fitted to: ring 10, K-sliced ring 11, split-K kernel 12)
inline long stream_cost(long blocks, long bytes_per_k, int k, int tenths) {
    return ((blocks + 255) / 256) * bytes_per_k * (long)k * tenths / 10;
}
// K slices meeting in the workspace: the seam in bytes of streaming (scripts/bench_gemm_shard.py, VARIANTS=4001,-1): slab stores ->
// ticket -> slab loads (one batch for mt <= 2, one per slice for mt = 4); measured 3-7 us: three dependent round trips
inline long seam_cost(int ks, int mt) {
    return ks <= 1 ? 0 : ((ks == 2 ? 150L : 250L) + (mt > 2 ? 40L * (ks - 2) : 0)) * 1024;
}

// What a search over RING_GEO x K slices switches on.  Three searches exist (below); where they differ the difference
// REPRODUCES what each did before they shared this code - nobody has measured whether it is wanted.
enum Mt8Rule {
    MT8_NEVER,        // <8,2> is not a candidate
    MT8_PER_GROUP,    // per-group only, un-split, at 65 .. 128 tokens: one level-2 dequant of a weight byte serves 128 tokens.
                      // Measured (scripts/gpu_mt8_ab.sh, g128): gate_up 28 672 x 4096 at M = 128 30.6 us against 35.6 for <4,4> x 2
                      // token blocks; per-channel it LOSES (28.5 vs 25.4 us: ring depth 3, nothing to share), K-sliced or four-unit
                      // forms lose everywhere (<8,4>: 60 us), for N <= 6144 the 64-token geometries fill the chip better
    MT8_FORCED_ONLY   // only as the forced geometry (measured: the 128-token geometry never wins as planes)
};
struct RingSearch {
    int max_ks;             // K slices tried: 1, 2, 4 up to this
    bool group_term;        // per-group: the level-2 dequant is VALU work per weight byte a workgroup streams (measured at M = 128,
                            // g128: qkv 16.0 us with (4,1) against 18.2 with the equal-bytes (2,2)) - a quarter of the weight bytes
    bool seam;              // K slices pay seam_cost (they meet in the workspace)
    bool plane_traffic;     // K slices pay their planes instead: written once, read once - 8 bytes per element and slice, weighted
                            // by the CU : HBM rate ratio
    Mt8Rule mt8;
    bool sentinel_rule;     // K slices of at most 32 768 k: the seam's sentinel must stay out of reach of a partial sum
    bool underfilled_only;  // K slices only where the un-sliced grid does not fill the 256 CUs
    int forced;             // only the geometry 100 * (ks - 1) + 10 * mt + wn is a candidate; -1 = all
};
struct RingChoice { long cost; int mt, wn, ks; };   // cost < 0: no geometry fits
inline RingChoice ring_search(const RingSearch& s, int mode, int M, int N, int K) {
    const int mt_all = (M + 15) / 16;
    RingChoice best = {-1, 0, 0, 1};
    for (int ks = 1; ks <= s.max_ks; ks *= 2)
        for (const RingGeo& g : RING_GEO) {
            const int mt = g.mt, wn = g.wn;
            if (mt == 8) {
                if (s.mt8 == MT8_NEVER || (s.mt8 == MT8_FORCED_ONLY && s.forced < 0)) continue;
                if (s.mt8 == MT8_PER_GROUP && (mode != 1 || ks > 1 || mt_all <= 4 || mt_all > 8)) continue;
            }
            if (!ring_fits(mt, wn, ks, N, K)) continue;
            if (s.forced >= 0 && s.forced != 100 * (ks - 1) + 10 * mt + wn) continue;
            if (s.sentinel_rule && ks > 1 && K / ks > 32768) continue;
            const int mb = (mt_all + mt - 1) / mt;
            const long tiles = (long)mb * (N / (64 * wn));
            if (s.underfilled_only && ks > 1 && tiles > 256) continue;
            const long pg = s.group_term && mode == 1 ? 8 * wn : 0;
            long cost = stream_cost(tiles * ks, 16 * mt + 32 * wn + pg, K / ks, ks > 1 ? 11 : 10);   // (K-sliced streams: 10 % extra)
            if (s.seam) cost += seam_cost(ks, mt);
            if (s.plane_traffic) cost += (long)ks * M * N * 8 / 256 * 23 / 10;
            if (best.cost < 0 || cost < best.cost) best = {cost, mt, wn, ks};
        }
    return best;
}
inline GemmPlan ring_plan(int M, int mt, int wn, int ks) { return {GEMM_RING, {mt, wn, ((M + 15) / 16 + mt - 1) / mt, ks}}; }

// ---- the split-K kernel's token tiles ----------------------------------------------------------------------------------------
// one workgroup per 64-channel unit: all tokens, up to 64
inline int splitk_whole_mtile(int M) { return M <= 16 ? 1 : M <= 32 ? 2 : M <= 48 ? 3 : 4; }
// few units: fewest token blocks that still give >= 192 workgroups (measured: N=6144 -> 2 blocks of 32, N=4096 -> 4 of 16)
inline int splitk_shared_mtile(int units, int mt_all) {
    for (int cand = 4; cand >= 1; cand >>= 1)
        if (cand <= mt_all && (long)units * ((mt_all + cand - 1) / cand) >= 192) return cand;
    return 1;
}

// ---- the plan -----------------------------------------------------------------------------------------------------------------
// The kernel choice for a validated shape (check_shape) with M > 0, from the shape and the selection hook `variant` alone; K
// slices assume the split-K workspace (ring_unsplit_plan is what runs without it).  act: `out` is [M, N/2] = silu(gate) * up
// of the stacked gate_up result (epilogue of the ring / tiled / wide kernels) - GEMM_NONE when no kernel with that epilogue
// serves the shape (the caller runs the two ops).
inline GemmPlan plan_w4a8(int mode, bool act, int M, int N, int K, int variant) {
    const Variant v{variant};
    const int units = N / 64, nsteps = K / 128, mt_all = (M + 15) / 16;

    // compute-bound shapes (prefill): LDS-tiled kernels, 256- or 128-token tiles, taken once the tiles fill the chip
    if (N % 256 == 0 && K >= 256 && K < (1 << 24) && offsets_fit(M, N, K)) {
        int tmt = v.tile_forced;
        if (!tmt && v.tile_rule) {
            const long nb = N / 256;
            // measured crossovers (scripts/bench_gemm_big.py, N=4096..28672): the tiles must (nearly) fill 256 CUs
            // (M >= 192: a 256-token tile must be mostly real tokens - without this bound every N >= 49 152 took the tiled
            // kernel even at M = 64 and ran at 2 TB/s)
            if (M >= 192 && ((M + 255) / 256) * nb >= 192) tmt = 8;
            else if (M >= 256 && ((M + 127) / 128) * nb >= (mode == 0 ? 96 : 192)) tmt = 4;
        }
        // 256-token tiles, PER-GROUP: the four-wave kernel (gemm_w4a8_wide.hip) - one level-2 dequant per weight byte for 256
        // tokens instead of two: +10 ... 18 % in-run (profiles/round5_wide_ab.txt: 4096^3 70.2 -> 64.0 us, 8192 x 4096 x 14336
        // 436 -> 369 us).  Per-channel the two tiles measure the same within +-3 % (both ~3.2 POPS marginal): the eight-wave
        // one stays.
        if (tmt == 8 && (v.wide_forced || (mode == 1 && !v.wide_barred))) return {GEMM_WIDE, {8}};
        if (tmt) return {GEMM_TILED, {tmt}};
    }

    // decode shapes: LDS-DMA ring kernel with operands read one stage ahead (gemm_w4a8_ring.hip)
    if (v.ring_forced) {
        if (act && v.ring_ks > 1) return {GEMM_NONE};
        if (!(ring_geometry_exists(v.ring_mt, v.ring_wn) && ring_fits(v.ring_mt, v.ring_wn, v.ring_ks, N, K) &&
              (v.ring_ks == 1 || K / v.ring_ks <= 32768)))
            return {GEMM_INVALID, {v.ring_mt, v.ring_wn, 0, v.ring_ks}};
        return ring_plan(M, v.ring_mt, v.ring_wn, v.ring_ks);
    }
    // Short K (< 1024) at M <= 64 stays on the split-K kernel (fixed costs).
    if (M <= 1024 && !(K < 1024 && M <= 64) && v.ring_rule && offsets_fit(M, N, K)) {
        // K slices (ksplit 2 / 4, int32 partial tiles meeting in a workspace, the last-dispatched slice finishes): fewer bytes
        // per CU when neither tokens nor channels can be cut further, against the seam's cost
        const RingSearch search = {v.k_slices && !act ? 4 : 1, /*group_term*/ v.group_term, /*seam*/ true, /*plane_traffic*/ false,
                                   v.mt8 ? MT8_PER_GROUP : MT8_NEVER, /*sentinel_rule*/ true, /*underfilled_only*/ true, -1};
        RingChoice c = ring_search(search, mode, M, N, K);
        // Measured override of the byte model (scripts/gpu_plan_check.sh): where the model takes <2,2> x 4 K slices over two token
        // blocks and <2,1> x 2 slices fills the chip with the same 256 workgroups, the latter is 3-7 % faster - a third of the slab
        // traffic, and the two token blocks share their weight stream in L2.  Llama-3-8B down_proj (4096 x 14336) at 33-64 tokens:
        // 14.4-14.7 vs 15.3-15.8 us per-channel, 19.6-19.9 vs 20.6-20.9 g128.  The model puts the two 1 KB apart and cannot be
        // tuned to separate them without flipping M = 32 (measured the other way).
        if (c.cost >= 0 && c.mt == 2 && c.wn == 2 && c.ks == 4 && (mt_all + 1) / 2 == 2 && (long)2 * units * 2 == 256 &&
            ring_fits(2, 1, 2, N, K) && v.down_override)
            c.wn = 1, c.ks = 2;
        // the older register-staged split-K kernel takes any K and cuts the tokens down to 16 per workgroup: same byte model,
        // ~20 % slower at equal bytes (measured) - it wins where K leaves the ring kernel only coarse geometries (Llama-2-7B
        // down_proj: K = 11 008 = 172 stages, two-unit workgroups only)
        if (c.cost >= 0 && !act && units < 256 && units % 8 == 0 && M > 16 && M <= 128) {
            const int mto = splitk_shared_mtile(units, mt_all);
            if (stream_cost((long)units * ((mt_all + mto - 1) / mto), 16 * mto + 32, K, 12) < c.cost) c.cost = -1;
        }
        if (c.cost >= 0) return ring_plan(M, c.mt, c.wn, c.ks);
    }
    if (act) return {GEMM_NONE};   // (the two older decode kernels have no activation epilogue)

    // many channels: LDS-shared activation tiles + LDS-DMA rings (gemm_w4a8_lds.hip)
    if (((((units >= 256 && M > 16) || M >= 384) && !v.pair_barred) || v.pair_forced) && N % 128 == 0 && K >= 256)
        return {GEMM_PAIR};

    // Split-K kernel (gemm_w4a8.hip), heuristic (measured, scripts/bench_gemm*.py): every 64-channel unit is one workgroup whose
    // waves split K (exact int32 reduction in LDS); with few units (N/64 < 256 = CUs) the tokens are split over workgroups as well
    // (XCD-aware mapping so that the co-streaming workgroups share an L2) - more CUs pull the same weight bytes, no reduction
    // traffic; cross-block split-K (S > 1) stays off: the release/acquire fences cost more than they save at these sizes.
    const bool few_units = units < 256 && units % 8 == 0 && M > 16;
    int mtile = few_units ? splitk_shared_mtile(units, mt_all) : splitk_whole_mtile(M);
    bool xcd_map = few_units && mtile < mt_all;
    int NW = nsteps >= 16 && mtile <= 2 ? 8 : nsteps >= 4 ? 4 : (nsteps >= 2 ? 2 : 1);
    int S = 1;
    if (v.splitk_code >= 0) {   // A/B: 100 * mtile_override + 10 * S + NW
        NW = v.splitk_code % 10;
        S = (v.splitk_code / 10) % 10;
        const int mo = v.splitk_code / 100;
        if (mo >= 1 && mo <= 4) mtile = mo, xcd_map = mo < mt_all;
        else if (mo == 9) mtile = splitk_whole_mtile(M), xcd_map = false;   // 9 = classic mapping, one workgroup per unit
        if (S < 1) S = 1;
        if (NW < 1) NW = 1;
        if (NW > (mtile <= 2 ? 8 : 4)) NW = mtile <= 2 ? 8 : 4;
        if (NW == 3 || NW == 5 || NW == 6 || NW == 7) NW = 4;
    }
    if (NW > nsteps) NW = 1;
    return {GEMM_SPLITK, {mtile, NW, S, xcd_map ? 1 : 0}};
}

// The best un-split ring geometry: what a K-sliced ring plan runs as when there is no workspace (e.g. first call inside a
// capture).  Always found: the K-sliced plan's own <mt, wn> fits un-split.  As before it shared the search: no per-group
// term and no <8,2> (with one slice the seam, the plane traffic and the K-slice rules have nothing to act on).
inline GemmPlan ring_unsplit_plan(int M, int N, int K) {
    const RingSearch search = {1, /*group_term*/ false, /*seam*/ false, /*plane_traffic*/ false, MT8_NEVER,
                               /*sentinel_rule*/ false, /*underfilled_only*/ false, -1};
    const RingChoice c = ring_search(search, 0, M, N, K);
    return ring_plan(M, c.mt, c.wn, 1);
}

// K-slice planes (gemm_w4a8.hip, qs_w4a8_*_gemm_planes): the ring kernel leaves its K slices as int32 planes [ks][M][N] for
// the row kernel that follows.  The ring byte model with the seam replaced by the planes' traffic.  As before it shared the
// search: the per-group term is always on (QS_GEMM_RING_NO_GROUP_TERM is not consulted), K slices are neither bounded by the
// sentinel rule (no sentinel: no seam) nor kept to under-filled grids, and <8,2> runs only when forced.
// GEMM_NONE: not available for the shape (the caller runs the GEMM + row kernel pair).
inline GemmPlan planes_plan(int mode, int M, int N, int K, int variant) {
    if (M < 1 || M > 1024 || N < 64 || N % 64 || K < 1024 || K % 128 || !offsets_fit(M, N, K)) return {GEMM_NONE};
    const RingSearch search = {4, /*group_term*/ true, /*seam*/ false, /*plane_traffic*/ true, MT8_FORCED_ONLY,
                               /*sentinel_rule*/ false, /*underfilled_only*/ false, Variant{variant}.planes_forced};
    const RingChoice c = ring_search(search, mode, M, N, K);
    return c.cost < 0 ? GemmPlan{GEMM_NONE} : ring_plan(M, c.mt, c.wn, c.ks);
}

}  // namespace gemm_plan
