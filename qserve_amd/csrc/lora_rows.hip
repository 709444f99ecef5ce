// lora_rows.hip -- multi-LoRA next to the W4A8 linears, for MI355X (gfx950): out[t, :] += scaling[a] * B[a] (A[a] x[t]) with a = the adapter
// of row t's SEQUENCE, on the int8 activations the base GEMM of the same linear read.  DESIGN.md 10 ("LoRA adapters"); the rule is the
// header comment of qs_lora_rows in include/qserve_amd.h.  Rows are sequence-major with rows_per_seq rows per sequence, so a TILE - up
// to 16 consecutive rows of ONE sequence - shares one adapter: a workgroup reads a slice of A or B once for the whole tile.  A tile whose
// adapter is outside 0 .. slots-1 leaves both kernels at once: nothing of its rows is read or written, no address is formed from the id.
// No atomics, no cross-workgroup waits inside a launch, no scratch; every sum has a fixed order, so results are bit-identical run to run
// and eager against graph replay.  This file holds TWO kernels:
//
//   lora_shrink_kernel   grid = (tiles, K slices of 512, groups of 64 rank rows), 256 threads.  t[j, row] = sum_k A[a, j, k] x[row, k] on
//              v_mfma_f32_16x16x32_f16: the M index is the rank row j (A operand: 16 bytes of A per lane, straight from memory), the N
//              index the tile's row (B operand: 8 int8 of x per lane, converted to fp16 - exact), so a result register holds four
//              consecutive j of one row.  fp16 x fp16 products are exact in float32; only the float32 additions round.  Wave w takes k
//              in [128 w, 128 w + 128) of the slice (four k-steps, all loads issued up front) for up to four 16-row j tiles; the four waves'
//              results meet in LDS (rows padded to 68 floats: the 16-byte stores of a wave fall on distinct banks) and are summed in wave
//              order into the workspace plane of the K slice: ws float32 [K slices, T, nseg * r].  LDS: 17 408 bytes.
//
//   lora_expand_kernel   grid = (tiles, N slices of 512), 256 threads, two adjacent output columns per thread.  First the tile's
//              t[row, j] = x_scale[row] * (sum of the K-slice planes, in slice order) is staged in LDS, all segments (at most 16 x 192
//              floats) - the thread's rows of out and its first 8 rank columns of B are requested before, their latency runs beside the
//              staging; then every thread takes the r values of B for each of its two columns, 8 at a time, and for every row of the tile
//              runs the float32 chain acc = fma(B[n, j], t[row, g r + j], acc) over j ascending - t comes from LDS as wave-wide
//              broadcasts, g is the segment of the thread's own columns (segment ends are multiples of 64: a pair never straddles one) -
//              and finally out = fp16(float(out) + scaling[a] * acc) as one 4-byte read-modify-write per row.  LDS: 12 288 bytes.
//
// The LDS bound of the file: 17 408 bytes per workgroup.
#include "common.h"

namespace {

constexpr int LR_THREADS = 256;
constexpr int LR_WAVES = LR_THREADS / 64;
constexpr int LR_TILE = 16;                          // rows of one sequence per workgroup (the N extent of the MFMA)
constexpr int LR_KSLICE = 512;                       // k per shrink workgroup: 128 per wave, four k-steps of 32
constexpr int LR_JGROUP = 64;                        // rank rows per shrink workgroup: four MFMA tiles of 16
constexpr int LR_RED_LD = LR_JGROUP + 4;             // floats per row of the cross-wave exchange (padded against bank conflicts)
constexpr int LR_NSLICE = 2 * LR_THREADS;            // output columns per expand workgroup
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

// grid = (tiles, K slices, j groups), 256 threads.  tps: tiles per sequence; R = nseg * r.  The launcher checks everything.
__global__ __launch_bounds__(LR_THREADS) void lora_shrink_kernel(const int8_t* __restrict__ x, long long x_stride,
                                                                 const _Float16* __restrict__ A, const int* __restrict__ seq_adapter,
                                                                 int slots, int K, int R, int rps, int tps, int T, float* __restrict__ ws) {
    __shared__ __attribute__((aligned(16))) float s_red[LR_WAVES][LR_TILE][LR_RED_LD];
    const int s = blockIdx.x / tps, ti = blockIdx.x - s * tps;
    const int a = seq_adapter[s];
    if (a < 0 || a >= slots) return;                     // the base model (workgroup-uniform)
    const int row0 = s * rps + ti * LR_TILE;
    const int rows = rps - ti * LR_TILE < LR_TILE ? rps - ti * LR_TILE : LR_TILE;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
    const int j0 = blockIdx.z * LR_JGROUP;
    const int k0 = blockIdx.y * LR_KSLICE + wave * (LR_KSLICE / LR_WAVES);
    v4f acc[4];
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) acc[jt] = v4f{0.f, 0.f, 0.f, 0.f};
    if (k0 < K) {                                        // (wave-uniform; K is a multiple of 128: a wave's range is whole or absent)
        h8 xb[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            v2u raw = {0u, 0u};
            if (c < rows) raw = *reinterpret_cast<const v2u*>(x + (size_t)(row0 + c) * x_stride + k0 + 32 * ks + 8 * g);
            xb[ks] = s8_to_h8(raw);
        }
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) {
            if (j0 + 16 * jt < R) {                      // (workgroup-uniform)
                const int j = j0 + 16 * jt + c;
                v4u ar[4];
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    ar[ks] = v4u{0u, 0u, 0u, 0u};
                    if (j < R) ar[ks] = *reinterpret_cast<const v4u*>(A + ((size_t)a * R + j) * K + k0 + 32 * ks + 8 * g);
                }
#pragma unroll
                for (int ks = 0; ks < 4; ++ks)
                    acc[jt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, ar[ks]), xb[ks], acc[jt], 0, 0, 0);
            }
        }
    }
    // a result register: row c of the tile, rank rows 16 jt + 4 g .. + 3
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) *reinterpret_cast<v4f*>(&s_red[wave][c][16 * jt + 4 * g]) = acc[jt];
    __syncthreads();
    const int t = tid >> 4, jq = (tid & 15) * 4;
    if (t < rows && j0 + jq < R) {                       // (R is a multiple of 8: four values are inside or outside together)
        v4f sum = *reinterpret_cast<const v4f*>(&s_red[0][t][jq]);
#pragma unroll
        for (int w = 1; w < LR_WAVES; ++w) sum += *reinterpret_cast<const v4f*>(&s_red[w][t][jq]);
        *reinterpret_cast<v4f*>(ws + ((size_t)blockIdx.y * T + row0 + t) * R + j0 + jq) = sum;
    }
}

// grid = (tiles, N slices), 256 threads.  e0, e1: the ends of segments 0 and 1 (INT_MAX where there is no such boundary).
__global__ __launch_bounds__(LR_THREADS) void lora_expand_kernel(_Float16* __restrict__ out, long long out_stride,
                                                                 const _Float16* __restrict__ x_scale, const _Float16* __restrict__ B,
                                                                 const float* __restrict__ scaling, const int* __restrict__ seq_adapter,
                                                                 int slots, int N, int r, int R, int rps, int tps, int T, int kslices, int e0,
                                                                 int e1, const float* __restrict__ ws) {
    __shared__ __attribute__((aligned(16))) float s_t[LR_TILE][LR_MAX_R];
    const int s = blockIdx.x / tps, ti = blockIdx.x - s * tps;
    const int a = seq_adapter[s];
    if (a < 0 || a >= slots) return;                     // the base model (workgroup-uniform)
    const int row0 = s * rps + ti * LR_TILE;
    const int rows = rps - ti * LR_TILE < LR_TILE ? rps - ti * LR_TILE : LR_TILE;
    const int tid = threadIdx.x;

    // what does not depend on the planes is requested first, so that its latency runs beside the staging: the thread's rows of `out`
    // and the first 8 rank columns of its two rows of B
    const int n = blockIdx.y * LR_NSLICE + 2 * tid;
    const bool mine = n < N;
    const _Float16* __restrict__ bp = B + ((size_t)a * N + (mine ? n : 0)) * r;
    u32 o[LR_TILE];
#pragma unroll
    for (int t = 0; t < LR_TILE; ++t) {
        o[t] = 0u;
        if (mine && t < rows) o[t] = *reinterpret_cast<const u32*>(out + (size_t)(row0 + t) * out_stride + n);
    }
    h8 b0 = {}, b1 = {};
    if (mine) {
        b0 = *reinterpret_cast<const h8*>(bp);
        b1 = *reinterpret_cast<const h8*>(bp + r);
    }

    // ---- 1. t[row, j] = x_scale[row] * (the K-slice planes summed in slice order), all segments
    const int q = R >> 2;
    for (int i = tid; i < rows * q; i += LR_THREADS) {
        const int t = i / q, j4 = (i - t * q) * 4;
        const float* p = ws + (size_t)(row0 + t) * R + j4;
        v4f sum = *reinterpret_cast<const v4f*>(p);
#pragma unroll 8
        for (int sl = 1; sl < kslices; ++sl) sum += *reinterpret_cast<const v4f*>(p + (size_t)sl * T * R);
        const float sx = (float)x_scale[row0 + t];
        *reinterpret_cast<v4f*>(&s_t[t][j4]) = sum * sx;
    }
    __syncthreads();

    // ---- 2. two columns per thread, every row of the tile
    if (!mine) return;
    const int seg = (n >= e0 ? 1 : 0) + (n >= e1 ? 1 : 0);
    const float sc = scaling[a];
    float acc0[LR_TILE], acc1[LR_TILE];
#pragma unroll
    for (int t = 0; t < LR_TILE; ++t) acc0[t] = acc1[t] = 0.f;
    for (int j0 = 0; j0 < r; j0 += 8) {
        h8 nb0 = b0, nb1 = b1;
        if (j0 + 8 < r) {                                // the next 8 rank columns, requested before this chunk's arithmetic
            nb0 = *reinterpret_cast<const h8*>(bp + j0 + 8);
            nb1 = *reinterpret_cast<const h8*>(bp + r + j0 + 8);
        }
        const float* sp = &s_t[0][seg * r + j0];
#pragma unroll
        for (int t = 0; t < LR_TILE; ++t) {
            if (t < rows) {                              // (workgroup-uniform)
                const v4f u = *reinterpret_cast<const v4f*>(sp + t * LR_MAX_R), v = *reinterpret_cast<const v4f*>(sp + t * LR_MAX_R + 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    acc0[t] = __builtin_fmaf((float)b0[e], u[e], acc0[t]);
                    acc1[t] = __builtin_fmaf((float)b1[e], u[e], acc1[t]);
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    acc0[t] = __builtin_fmaf((float)b0[4 + e], v[e], acc0[t]);
                    acc1[t] = __builtin_fmaf((float)b1[4 + e], v[e], acc1[t]);
                }
            }
        }
        b0 = nb0;
        b1 = nb1;
    }
#pragma unroll
    for (int t = 0; t < LR_TILE; ++t) {
        if (t < rows) {
            const h2 old = __builtin_bit_cast(h2, o[t]);
            const float y0 = __builtin_fmaf(sc, acc0[t], (float)old[0]), y1 = __builtin_fmaf(sc, acc1[t], (float)old[1]);
            *reinterpret_cast<u32*>(out + (size_t)(row0 + t) * out_stride + n) = pack_h2(y0, y1);
        }
    }
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

inline bool rank_ok(int r) { return r == 8 || r == 16 || r == 32 || r == 64; }

inline int64_t workspace_bytes(int T, int K, int r, int nseg) {
    return (int64_t)((K + LR_KSLICE - 1) / LR_KSLICE) * T * nseg * r * (int64_t)sizeof(float);
}

}  // namespace

extern "C" int64_t qs_lora_rows_workspace(int T, int K, int r, int nseg) {
    QS_REQUIRE(T >= 0 && T <= LR_MAX_ROWS && K >= 128 && K <= LR_MAX_K && K % 128 == 0 && rank_ok(r) && nseg >= 1 && nseg <= LR_MAX_SEG,
               "lora_rows_workspace: T=%d (0 .. %d), K=%d (a multiple of 128, <= %d), r=%d (8, 16, 32, 64), nseg=%d (1 .. 3)", T,
               LR_MAX_ROWS, K, LR_MAX_K, r, nseg);
    return workspace_bytes(T, K, r, nseg);
}

extern "C" int qs_lora_rows(void* out, int64_t out_stride, const int8_t* x, int64_t x_stride, const void* x_scale, const void* A,
                            const void* B, const float* scaling, const int32_t* seq_adapter, int slots, int T, int K, int N, int r,
                            int rows_per_seq, int nseg, int seg_end0, int seg_end1, int seg_end2, void* workspace, int64_t workspace_size,
                            qs_stream_t stream) {
    QS_REQUIRE(out && x && x_scale && A && B && scaling && seq_adapter && workspace, "lora_rows: null pointer");
    QS_REQUIRE(rank_ok(r), "lora_rows: r=%d (8, 16, 32 or 64)", r);
    QS_REQUIRE(K >= 128 && K <= LR_MAX_K && K % 128 == 0, "lora_rows: K=%d (a multiple of 128, 128 .. %d)", K, LR_MAX_K);
    QS_REQUIRE(N >= 64 && N <= LR_MAX_N && N % 64 == 0, "lora_rows: N=%d (a multiple of 64, 64 .. %d)", N, LR_MAX_N);
    QS_REQUIRE(nseg >= 1 && nseg <= LR_MAX_SEG, "lora_rows: nseg=%d (1 .. %d)", nseg, LR_MAX_SEG);
    const int ends[LR_MAX_SEG] = {seg_end0, seg_end1, seg_end2};
    for (int g = 0, prev = 0; g < nseg; prev = ends[g++])
        QS_REQUIRE(ends[g] > prev && ends[g] % 64 == 0, "lora_rows: segment end %d = %d (ascending multiples of 64)", g, ends[g]);
    QS_REQUIRE(ends[nseg - 1] == N, "lora_rows: the last segment ends at %d, N=%d", ends[nseg - 1], N);
    QS_REQUIRE(slots >= 1, "lora_rows: slots=%d (>= 1)", slots);
    QS_REQUIRE(T >= 0 && T <= LR_MAX_ROWS && rows_per_seq >= 1 && T % rows_per_seq == 0,
               "lora_rows: T=%d (0 .. %d) must be a multiple of rows_per_seq=%d (>= 1)", T, LR_MAX_ROWS, rows_per_seq);
    QS_REQUIRE(x_stride >= K && x_stride % 16 == 0 && out_stride >= N && out_stride % 8 == 0,
               "lora_rows: x stride %lld (>= K=%d, a multiple of 16), out stride %lld (>= N=%d, a multiple of 8)", (long long)x_stride, K,
               (long long)out_stride, N);
    QS_REQUIRE(aligned(out, 16) && aligned(x, 16) && aligned(A, 16) && aligned(B, 16) && aligned(workspace, 16) && aligned(x_scale, 2) &&
                   aligned(scaling, 4) && aligned(seq_adapter, 4),
               "lora_rows: out, x, A, B and the workspace must be 16-byte, scaling and seq_adapter 4-byte, x_scale 2-byte aligned");
    QS_REQUIRE(workspace_size >= workspace_bytes(T, K, r, nseg), "lora_rows: the workspace holds %lld bytes, %lld are needed",
               (long long)workspace_size, (long long)workspace_bytes(T, K, r, nseg));
    if (T == 0) return QS_OK;
    const int R = nseg * r, tps = (rows_per_seq + LR_TILE - 1) / LR_TILE, tiles = T / rows_per_seq * tps;
    const int kslices = (K + LR_KSLICE - 1) / LR_KSLICE;
    const int e0 = nseg >= 2 ? ends[0] : INT32_MAX, e1 = nseg >= 3 ? ends[1] : INT32_MAX;
    hipLaunchKernelGGL(lora_shrink_kernel, dim3(tiles, kslices, (R + LR_JGROUP - 1) / LR_JGROUP), dim3(LR_THREADS), 0, (hipStream_t)stream, x,
                       (long long)x_stride, (const _Float16*)A, seq_adapter, slots, K, R, rows_per_seq, tps, T, (float*)workspace);
    int rc = qs_launch_status("lora_rows (shrink)");
    if (rc != QS_OK) return rc;
    hipLaunchKernelGGL(lora_expand_kernel, dim3(tiles, (N + LR_NSLICE - 1) / LR_NSLICE), dim3(LR_THREADS), 0, (hipStream_t)stream,
                       (_Float16*)out, (long long)out_stride, (const _Float16*)x_scale, (const _Float16*)B, scaling, seq_adapter, slots, N, r,
                       R, rows_per_seq, tps, T, kslices, e0, e1, (const float*)workspace);
    return qs_launch_status("lora_rows (expand)");
}
