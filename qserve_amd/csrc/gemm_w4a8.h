// gemm_w4a8.h -- what the five W4A8 GEMM translation units (gemm_w4a8{,_ring,_tiled,_wide,_lds}.hip) share on the host side: the
// argument record every host function passes down to its hipLaunchKernelGGL line, the four family launchers the dispatcher
// (gemm_w4a8.hip) calls, and the flag words qs_set_gemm_variant sets.  Internal: not part of the C ABI.
#pragma once
#include "common.h"

// One GEMM problem.  The extern "C" entries fill it field by field (the ABI's `const void*` half pointers are typed here, once);
// kernels keep their own parameter lists - the record is unpacked at the launch line.
struct GemmArgs {
    const int8_t* A;          // [M, K] activations
    const uint8_t* W;         // packed weights (gemm_w4a8.hip header)
    const int8_t* zeros;      // per-group only: [K/128, N]
    const int8_t* scales8;    // per-group only: [K/128, N]
    const __half* wscales;    // [N]     } null for the int32 output kinds
    const __half* ascales;    // [M]     }
    const __half* wszs;       // per-channel only: [N]
    const __half* assums;     // per-channel only: [M]
    void* out;                // fp16 [M, N] | int32 [M, N] | fp16 [M, N/2] (silu * mul) | int32 planes [ks, M, N]: the output kind
    int M, N, K;
    hipStream_t stream;
};

// Family launchers.  mode 0 = per-channel, 1 = per-group(128); outk 0 = fp16 epilogue, 1 = raw int32 accumulators, 2 = fp16
// silu(gate) * up of a stacked gate_up (ring, tiled, wide), 3 = int32 K-slice planes (ring).  A (mode, outk, geometry) a family
// is not built for is QS_ENOSUP, never another kernel.  The shape preconditions are the planner's (gemm_plan.h).
int qs_launch_gemm_pair(int mode, int outk, const GemmArgs& a);                        // gemm_w4a8_lds.hip: N % 128 == 0, K >= 256
// gemm_w4a8_ring.hip: mt m-tiles x wn units per workgroup (gemm_plan.h RING_GEO), mblocks token blocks, ksplit K slices
// (1 = none; > 1 with outk 0 / 1 needs the slabs and counters of the split-K workspace, gemm_w4a8.hip)
int qs_launch_gemm_ring(int mode, int outk, int mt, int wn, const GemmArgs& a, int mblocks, int ksplit, int* slabs,
                        unsigned* counters);
int qs_launch_gemm_tiled(int mode, int outk, const GemmArgs& a, int mtile);            // gemm_w4a8_tiled.hip: m-tiles per wave 8 / 4
int qs_launch_gemm_wide(int mode, int outk, const GemmArgs& a, int persist_mode);      // gemm_w4a8_wide.hip

// Flag words of qs_set_gemm_variant's sticky families (include/qserve_amd.h qs_gemm_variant_code), defined where they are read
extern qs_flag g_tiled_dbg;    // gemm_w4a8_tiled.hip: timing experiments (3100 + bits; also read by the pair launcher)
extern qs_flag g_tiled_order;  // gemm_w4a8_tiled.hip: tile order / persistence A/B (3200 + 10 * p + mode)
extern qs_flag g_wide_order;   // gemm_w4a8_wide.hip: the same switch for the four-wave kernel
extern qs_flag g_wide_dbg;     // gemm_w4a8_wide.hip: timing experiments (3400 + bits; QS_TIMING builds only)
extern qs_flag g_ring_flags;   // gemm_w4a8_ring.hip: A/B switches of the decode kernel (5000 + bits), results unchanged
extern qs_flag g_act_off;      // gemm_w4a8.hip: 3301 / 3300: gate_up + silu always as two launches / default
