// lora_common.h -- what the three forms of the LoRA row update share: the rows and the grouped form (lora_rows.hip: 16-row tiles of one
// sequence's / one adapter's rows) and the prompt form (lora_prompt.hip: 64-row tiles of one sequence).  The limits, the workspace
// size, the int8 -> fp16 conversion of the shrink's operand, the tile of consecutive rows of one sequence, the two steps an expand
// kernel runs around its own loop - staging t, landing a pair of columns - and the host prologue of qs_lora_rows /
// qs_lora_rows_grouped / qs_lora_rows_prompt (include/qserve_amd.h): the argument rules and the derived sizes, written once; every entry
// answers them before any device call, under its own name.
#pragma once
#include "common.h"

namespace {

constexpr int LR_THREADS = 256;
constexpr int LR_WAVES = LR_THREADS / 64;
constexpr int LR_TILE = 16;                          // rows per workgroup (the N extent of the MFMA)
constexpr int LR_KSLICE = 512;                       // k per shrink workgroup: 128 per wave, four k-steps of 32
constexpr int LR_JGROUP = 64;                        // rank rows per shrink workgroup: four MFMA tiles of 16
constexpr int LR_RED_LD = LR_JGROUP + 4;             // floats per row of the cross-wave exchange (padded against bank conflicts)
constexpr int LR_NSLICE = 2 * LR_THREADS;            // output columns per expand workgroup (and per round of one that walks slices)
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

// A tile of up to ROWS consecutive rows of ONE sequence: tile blockIdx.x % tps of sequence blockIdx.x / tps (tps: tiles per sequence),
// the last tile of a sequence short.  rows == 0: the sequence's id is outside 0 .. slots-1 (the base model) - the workgroup leaves, and
// no address is formed from the id.  Workgroup-uniform.  The prompt form's tile; the rows form's kernels compute the same in place.
template <int ROWS>
struct SeqTile {
    int a;       // the adapter
    int rows;    // rows of the tile, 1 .. ROWS; 0: no tile, leave
    int row0;    // the tile's first row in the batch
    __device__ __forceinline__ SeqTile(const int* __restrict__ seq_adapter, int slots, int rps, int tps) {
        const int s = blockIdx.x / tps, ti = blockIdx.x - s * tps;
        a = seq_adapter[s];
        row0 = s * rps + ti * ROWS;
        rows = a < 0 || a >= slots ? 0 : rps - ti * ROWS < ROWS ? rps - ti * ROWS : ROWS;
    }
    __device__ __forceinline__ int row(int i) const { return row0 + i; }   // row i (< rows) of the tile, in the batch
};

// A float32 value the compiler has to produce as such.  The rule's last step is fp16(fmaf(scaling, acc, float(old))): a float32 fma, then
// the rounding to fp16.  Left alone the compiler folds the two into v_fma_mixlo_f16 / v_fma_mixhi_f16 - ONE rounding, which differs
// from the rule's two in about one element of 20 000 by an fp16 ulp (found when the grouped form was first compared with the rows form).
__device__ __forceinline__ float as_f32(float v) {
    asm volatile("" : "+v"(v));
    return v;
}

// The landing step of every expand kernel, and the only place where the rule's last two roundings are written: the two adjacent
// columns `old` of out (one 4-byte word) become fp16(fmaf(scaling, acc, float(old))).
__device__ __forceinline__ u32 lora_land(u32 old, float sc, float acc0, float acc1) {
    const h2 o = __builtin_bit_cast(h2, old);
    const float y0 = as_f32(__builtin_fmaf(sc, acc0, (float)o[0])), y1 = as_f32(__builtin_fmaf(sc, acc1, (float)o[1]));
    return pack_h2(y0, y1);
}

// The staging step of the grouped and the prompt expand: s_t[i * ld + j] = x_scale[row] * (the K-slice planes of row, added in slice
// order) for row = tl.row(i), i < tl.rows, j < R (all segments; R is a multiple of 8).  By the whole workgroup; the caller's barrier
// follows.  The rows form's expand keeps its own lines: on this helper and SeqTile it ran 1 % slower in the median
// (profiles/lora_one_body.txt).
template <class Tile>
__device__ __forceinline__ void lora_stage(float* __restrict__ s_t, int ld, const Tile& tl, int R, int T, int kslices,
                                           const float* __restrict__ ws, const _Float16* __restrict__ x_scale) {
    const int q = R >> 2;
    for (int i = threadIdx.x; i < tl.rows * q; i += LR_THREADS) {
        const int t = i / q, j4 = (i - t * q) * 4;
        const size_t row = tl.row(t);
        const float* p = ws + row * R + j4;
        v4f sum = *reinterpret_cast<const v4f*>(p);
#pragma unroll 8
        for (int sl = 1; sl < kslices; ++sl) sum += *reinterpret_cast<const v4f*>(p + (size_t)sl * T * R);
        const float sx = (float)x_scale[row];
        *reinterpret_cast<v4f*>(&s_t[t * ld + j4]) = sum * sx;
    }
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

// What every entry derives from its arguments once they passed: R = nseg * r rank rows of all segments, the K slices of the shrink
// and the workspace, the column slices of the expand, e0 / e1 = the ends of segments 0 and 1 (INT32_MAX where there is no such
// boundary), and the pointers under the types the kernels take.
struct LoraCall {
    int R, kslices, nslices, e0, e1;
    _Float16* out;
    const _Float16 *x_scale, *A, *B;
    float* ws;
};

// The host prologue of the three entries: lora_check_args under the name `what`, then the record.  QS_OK or QS_EINVAL.
inline int lora_prologue(const char* what, LoraCall& c, void* out, int64_t out_stride, const int8_t* x, int64_t x_stride, const void* x_scale,
                         const void* A, const void* B, const float* scaling, const int32_t* seq_adapter, int slots, int T, int K, int N,
                         int r, int rows_per_seq, int nseg, int seg_end0, int seg_end1, int seg_end2, void* workspace,
                         int64_t workspace_size) {
    const int ends[LR_MAX_SEG] = {seg_end0, seg_end1, seg_end2};
    const int rc = lora_check_args(what, out, out_stride, x, x_stride, x_scale, A, B, scaling, seq_adapter, slots, T, K, N, r, rows_per_seq,
                                   nseg, ends, workspace, workspace_size);
    if (rc != QS_OK) return rc;
    c = LoraCall{nseg * r, (K + LR_KSLICE - 1) / LR_KSLICE, (N + LR_NSLICE - 1) / LR_NSLICE, nseg >= 2 ? ends[0] : INT32_MAX,
                 nseg >= 3 ? ends[1] : INT32_MAX, (_Float16*)out, (const _Float16*)x_scale, (const _Float16*)A, (const _Float16*)B,
                 (float*)workspace};
    return QS_OK;
}

}  // namespace
