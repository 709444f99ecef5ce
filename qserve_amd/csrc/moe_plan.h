// moe_plan.h -- the geometry of the grouped (mixture-of-experts) W4A8 GEMM.  Plain C++17 next to gemm_plan.h: no HIP, no device
// access, no global state - a plan is a function of (P, E, N, K) alone, P = sorted rows (tokens x experts per token), so it can be
// pinned on a machine without a GPU (tests/golden/moe_plan_table.json through qs_moe_gemm_plan).  gemm_w4a8_moe.hip launches what
// this returns.  Every plan computes the same bits: integer accumulation is exact and the epilogue is per element.
#pragma once

namespace moe_plan {

struct MoePlan {
    int mt;        // m-tiles (16 sorted rows each) of a workgroup: 1, 2 or 4
    int nw;        // waves of a workgroup, splitting the K/128 k-steps round-robin: 1, 2, 4 or 8 (a wave may get no step)
    int mblocks;   // row blocks launched: ceil(P / (16 mt)) + E - 1, a bound that holds for EVERY routing (below)
    int units;     // 64-channel units: N / 64
};

// Row blocks: expert e with c_e > 0 rows needs ceil(c_e / R) = floor((c_e - 1) / R) + 1 blocks of R = 16 mt rows.  Over the n <= E
// non-empty experts that sums to at most floor((P - n) / R) + n, which grows with n and is floor((P - E) / R) + E <=
// floor((P - 1) / R) + E = ceil(P / R) + E - 1 at n = E (reached by E - 1 single rows and the rest on one expert).  The bound holds
// for every routing, so the host never reads one.
inline int row_blocks(int P, int E, int mt) { return P <= 0 ? 0 : (P + 16 * mt - 1) / (16 * mt) + E - 1; }

// m-tiles from the EXPECTED rows per expert, ceil(P / E): a workgroup streams its expert's weights once for its 16 mt rows, so the
// tile should cover the typical expert in one block and no more (rows past the expert's range are computed and dropped).  4 is the
// largest tile the register-staged kernel holds at two workgroups per CU (gemm_w4a8.hip).
inline int moe_mt(int P, int E) {
    const int avg = E > 0 ? (P + E - 1) / E : P;
    return avg <= 16 ? 1 : avg <= 32 ? 2 : 4;
}
// waves: the split-K kernel's rule (gemm_plan.h): 8 where K is long and the tile small, else 4, 2 for two k-steps, 1 for one
inline int moe_nw(int K, int mt) {
    const int nsteps = K / 128;
    return nsteps >= 16 && mt <= 2 ? 8 : nsteps >= 3 ? 4 : nsteps >= 2 ? 2 : 1;
}
inline MoePlan plan_moe(int P, int E, int N, int K) {
    const int mt = moe_mt(P, E);
    return {mt, moe_nw(K, mt), row_blocks(P, E, mt), N / 64};
}

// ---- the compute-bound tile (gemm_w4a8_moe_tiled.hip): a workgroup owns (expert, 128 sorted rows, 256 channels) and walks K in
// stages of 64 through LDS.  plan_moe above describes the streaming form and is what it was.
constexpr int TILED_ROWS = 128;       // sorted rows of a tile
constexpr int TILED_CHANNELS = 256;   // channels of a tile
struct MoeTiledPlan {
    int rows;      // sorted rows per tile: 128
    int ntiles;    // channel tiles: N / 256
    int rblocks;   // row blocks launched: ceil(P / 128) + E - 1 (the bound argument of row_blocks with R = 128)
    int stages;    // pipeline stages of 64 k: K / 64
};
inline int row_blocks_tiled(int P, int E) { return P <= 0 ? 0 : (P + TILED_ROWS - 1) / TILED_ROWS + E - 1; }
inline MoeTiledPlan plan_moe_tiled(int P, int E, int N, int K) { return {TILED_ROWS, N / TILED_CHANNELS, row_blocks_tiled(P, E), K / 64}; }

// What the tile serves at all: whole channel tiles, at least the four stages its pipeline fill requests, and 32-bit per-lane offsets
// into the activations (x_rows rows of x_stride bytes) and into ONE expert's packed weights (the expert's base is a scalar).
inline bool tiled_serves(long long x_rows, long long x_stride, int N, int K) {
    return N % TILED_CHANNELS == 0 && K >= 256 && x_rows * x_stride < (1ll << 32) && (long long)N * K / 2 < (1ll << 32);
}

// The form the entries take for (P, E, N, K).  TILED_MIN_ROWS is the smallest expected rows per expert, ceil(P / E), of the measured sweep
// 32, 64, ... 2048 from which the tile beat the streaming kernel by more than the sweep's run-to-run spread at both Mixtral shapes
// (gate_up 28672 x 4096, down 4096 x 14336) and for both weight modes (profiles/moe_tiled.txt, "crossover"): per-channel the tile
// wins from 64 rows on (0.72 / 0.81 of the streaming time, spread 0.12); per-group-128 it wins at 128, loses at 256 for down (368
// tiles: a second round on 256 CUs) and wins from 512 on (0.69 / 0.87, spread 0.05).  The form has no mode argument, so the later of
// the two crossovers is the threshold.  The pure planner takes dense rows (x_stride = K, x_rows = P) for the offset rule; the
// entries apply it to the strides they are given.
constexpr int TILED_MIN_ROWS = 512;
enum MoeForm { MOE_STREAMING = 0, MOE_TILED = 1 };
inline MoeForm moe_form(int P, int E, int N, int K) {
    if (P <= 0 || E <= 0 || !tiled_serves(P, K, N, K)) return MOE_STREAMING;
    return (P + E - 1) / E >= TILED_MIN_ROWS ? MOE_TILED : MOE_STREAMING;
}

}  // namespace moe_plan
