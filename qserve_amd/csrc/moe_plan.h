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

}  // namespace moe_plan
