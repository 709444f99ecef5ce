// lora_common.h -- what the two forms of the LoRA row update share: lora_rows.hip (tiles of one sequence's rows) and lora_grouped.hip
// (tiles of one adapter's rows).  The limits, the workspace size, the int8 -> fp16 conversion of the shrink's operand, and the
// argument rules of qs_lora_rows / qs_lora_rows_grouped (include/qserve_amd.h), written once: both entries answer them before any
// device call, under their own name.
#pragma once
#include "common.h"

namespace {

constexpr int LR_THREADS = 256;
constexpr int LR_WAVES = LR_THREADS / 64;
constexpr int LR_TILE = 16;                          // rows per workgroup (the N extent of the MFMA)
constexpr int LR_KSLICE = 512;                       // k per shrink workgroup: 128 per wave, four k-steps of 32
constexpr int LR_JGROUP = 64;                        // rank rows per shrink workgroup: four MFMA tiles of 16
constexpr int LR_RED_LD = LR_JGROUP + 4;             // floats per row of the cross-wave exchange (padded against bank conflicts)
constexpr int LR_NSLICE = 2 * LR_THREADS;            // output columns per expand workgroup (and per round of a grouped one)
constexpr int LR_MAX_SEG = 3;
constexpr int LR_MAX_RANK = 64;
constexpr int LR_MAX_R = LR_MAX_SEG * LR_MAX_RANK;   // rank rows of all segments
constexpr int LR_MAX_ROWS = 1 << 24;
constexpr int LR_MAX_K = 1 << 20;
constexpr int LR_MAX_N = 1 << 22;

// 8 int8 -> 8 fp16 (exact)
__device__ __forceinline__ h8 s8_to_h8(v2u v) {
    h8 r;
#pragma unroll
    for (int e = 0; e < 8; ++e) r[e] = (_Float16)(short)(signed char)((v[e >> 2] >> (8 * (e & 3))) & 0xFFu);
    return r;
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

inline bool rank_ok(int r) { return r == 8 || r == 16 || r == 32 || r == 64; }

inline int64_t workspace_bytes(int T, int K, int r, int nseg) {
    return (int64_t)((K + LR_KSLICE - 1) / LR_KSLICE) * T * nseg * r * (int64_t)sizeof(float);
}

// The argument rules of a LoRA rows call, `what` the entry's name in the message.  QS_OK, or QS_EINVAL with the error text set.
inline int lora_check_args(const char* what, const void* out, int64_t out_stride, const int8_t* x, int64_t x_stride, const void* x_scale,
                           const void* A, const void* B, const float* scaling, const int32_t* seq_adapter, int slots, int T, int K, int N,
                           int r, int rows_per_seq, int nseg, const int (&ends)[LR_MAX_SEG], const void* workspace, int64_t workspace_size) {
    QS_REQUIRE(out && x && x_scale && A && B && scaling && seq_adapter && workspace, "%s: null pointer", what);
    QS_REQUIRE(rank_ok(r), "%s: r=%d (8, 16, 32 or 64)", what, r);
    QS_REQUIRE(K >= 128 && K <= LR_MAX_K && K % 128 == 0, "%s: K=%d (a multiple of 128, 128 .. %d)", what, K, LR_MAX_K);
    QS_REQUIRE(N >= 64 && N <= LR_MAX_N && N % 64 == 0, "%s: N=%d (a multiple of 64, 64 .. %d)", what, N, LR_MAX_N);
    QS_REQUIRE(nseg >= 1 && nseg <= LR_MAX_SEG, "%s: nseg=%d (1 .. %d)", what, nseg, LR_MAX_SEG);
    for (int g = 0, prev = 0; g < nseg; prev = ends[g++])
        QS_REQUIRE(ends[g] > prev && ends[g] % 64 == 0, "%s: segment end %d = %d (ascending multiples of 64)", what, g, ends[g]);
    QS_REQUIRE(ends[nseg - 1] == N, "%s: the last segment ends at %d, N=%d", what, ends[nseg - 1], N);
    QS_REQUIRE(slots >= 1, "%s: slots=%d (>= 1)", what, slots);
    QS_REQUIRE(T >= 0 && T <= LR_MAX_ROWS && rows_per_seq >= 1 && T % rows_per_seq == 0,
               "%s: T=%d (0 .. %d) must be a multiple of rows_per_seq=%d (>= 1)", what, T, LR_MAX_ROWS, rows_per_seq);
    QS_REQUIRE(x_stride >= K && x_stride % 16 == 0 && out_stride >= N && out_stride % 8 == 0,
               "%s: x stride %lld (>= K=%d, a multiple of 16), out stride %lld (>= N=%d, a multiple of 8)", what, (long long)x_stride, K,
               (long long)out_stride, N);
    QS_REQUIRE(aligned(out, 16) && aligned(x, 16) && aligned(A, 16) && aligned(B, 16) && aligned(workspace, 16) && aligned(x_scale, 2) &&
                   aligned(scaling, 4) && aligned(seq_adapter, 4),
               "%s: out, x, A, B and the workspace must be 16-byte, scaling and seq_adapter 4-byte, x_scale 2-byte aligned", what);
    QS_REQUIRE(workspace_size >= workspace_bytes(T, K, r, nseg), "%s: the workspace holds %lld bytes, %lld are needed", what,
               (long long)workspace_size, (long long)workspace_bytes(T, K, r, nseg));
    return QS_OK;
}

}  // namespace
