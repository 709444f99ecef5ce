// gemm_w4a8_moe.h -- what the two grouped W4A8 GEMM translation units (gemm_w4a8_moe.hip: the entries, their argument checks and the
// weight-streaming kernel; gemm_w4a8_moe_tiled.hip: the compute-bound tile) share on the host side.  Internal: not part of the C ABI.
#pragma once
#include "common.h"

// One grouped GEMM problem (include/qserve_amd.h, the block above qs_moe_gemm_plan).  The extern "C" entries fill it; the argument
// rules are checked once, in gemm_w4a8_moe.hip, before either form is launched.
struct MoeArgs {
    const int8_t* x;
    int64_t x_stride;
    int x_rows;
    const int32_t *row_src, *offsets;
    const int8_t *qweight, *zeros, *scales8;
    const void *wscales, *ascales, *wszs, *assums;
    void* out;
    int64_t out_stride;
    int P, E, N, K;
    hipStream_t stream;
};

// gemm_w4a8_moe_tiled.hip: mode 0 = per-channel, 1 = per-group(128).  Preconditions (moe_plan::tiled_serves, checked by the caller):
// N % 256 == 0, K >= 256, x_rows * x_stride and one expert's N * K / 2 below 2^32; P >= 1.
int qs_launch_moe_tiled(int mode, const MoeArgs& a);
