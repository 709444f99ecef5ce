// lora_grouped.hip -- the GROUPED form of the multi-LoRA row update of lora_rows.hip, for MI355X (gfx950): the same rule (qs_lora_rows in
// include/qserve_amd.h), the same bits, but a TILE is 16 rows of one ADAPTER, wherever they sit in the batch, not up to 16 rows of one
// sequence.  DESIGN.md 10 ("Grouped rows").  The rows of adapter a are all rows t with seq_adapter[t / rows_per_seq] == a in ascending t;
// tile i of adapter a is rows 16 i .. 16 i + 15 of that list; the tiles of adapter 0 come first in the grid, then those of adapter 1 ...
// At rows_per_seq < 16 the rows form's tiles are mostly padding and A / B are fetched again for every sequence; here every column of
// the MFMA is a real row and a slice of A or B is read once per 16 rows of its adapter.  Rows of an id outside 0 .. slots-1 belong to no
// tile: nothing of them is read or written, no address is formed from the id.
//
// Every workgroup FINDS ITS OWN TILE on the device (find_tile; nothing of the ids reaches the host, so a captured graph follows ids
// changed in place).  The grid's tile extent is lora_plan.h's bound ceil(T / 16) + min(slots, S) - 1, S = T / rows_per_seq sequences;
// a workgroup past the last real tile leaves at once.  The scan reads the S ids, not the T rows: wave w counts the ids of ITS
// contiguous quarter of the sequences per adapter into its own row of LDS counters (integer adds: a count has no order); after one
// barrier every wave adds the four rows per adapter (lane = adapter), turns rows into tiles, takes an inclusive prefix over the lanes
// and picks with one ballot the adapter whose tile range holds blockIdx.x - that gives (adapter, first rank); the wave whose quarter
// holds sequences of that rank range walks it again, 64 ids per round, and a ballot prefix over the matches, continued from the
// counts of the earlier quarters, places match number m at s_seq[m - first match] - ascending, so membership is deterministic; a
// second barrier, and row i of the tile is s_seq[(rank + i) / rows_per_seq - first match] * rows_per_seq + (rank + i) % rows_per_seq.
// No permutation is stored: both kernels scan for themselves, and the workspace is exactly the rows form's (qs_lora_rows_workspace:
// float32 K-slice planes [K slices, T, nseg * r], indexed by the ORIGINAL row).
//
// Same bits as lora_rows.hip, element for element: per row and rank row chains of four MFMA k-steps over each 128-chunk of K from
// +0.0; the four chunk sums of a 512-slice added in chunk order; the slices added in slice order; one multiply by float(x_scale);
// acc = fmaf(float(B[n, j]), t_j, acc) over j ascending; fp16(fmaf(scaling, acc, float(old))).  An MFMA column depends on its own
// operand column only, so which rows share a tile does not change a row's value.  Every float32 step is an explicit operation (an add
// or a multiply alone, or __builtin_fmaf), and the last fmaf is held as a float32 value (as_f32) so that it is not folded into the
// fp16 rounding: nothing the compiler contracts in one file and not in the other.  No atomic decides an order, no cross-workgroup wait
// inside a launch, no scratch.  This file holds TWO kernels:
//
//   lora_grouped_shrink_kernel   grid = (tile bound, K slices of 512, groups of 64 rank rows), 256 threads.  After find_tile: the rows
//              form's shrink on v_mfma_f32_16x16x32_f16 - M the rank row (A straight from memory, 16 bytes per lane), N the tile's row
//              (8 int8 of x per lane GATHERED through the tile's row list, int8 -> fp16 exactly), wave w on k in [128 w, 128 w + 128)
//              of the slice; the four waves' results meet in LDS (rows padded to 68 floats) and are summed in wave order into the
//              plane of the K slice at the gathered row.  One workgroup per (tile, 512-slice) and NOT per (tile, 128-chunk): the
//              chunk sums of a slice have to be added in chunk order before they land in the slice's plane; workgroups per chunk
//              would need a plane per chunk - four times the workspace the rows form's contract fixes - or an ordered hand-over
//              between workgroups, which is ruled out.  So the finer split was not built; few-tile calls fill the CUs through the K
//              slices and rank groups (profiles/lora_grouped.txt).  LDS: 17 408 + 1 024 (counters) + 64 (sequences) = 18 496 bytes.
//
//   lora_grouped_expand_kernel   grid = (tile bound, ysplit), 256 threads, two adjacent output columns per thread.  After find_tile: the
//              rows of out and the first 8 rank columns of B for the workgroup's first column slice are requested; the tile's
//              t[row, j] = x_scale[row] * (the K-slice planes summed in slice order) is staged in LDS, all segments, from the gathered
//              rows; then the workgroup walks the column slices blockIdx.y, blockIdx.y + ysplit, ... of 512 columns (lora_plan.h: with
//              many tiles a workgroup keeps its tile for several slices, so the id scan and the staging are paid once for them): every
//              thread holds B of the tile's adapter for its two columns in registers, 8 rank columns at a time - read once per 16 rows
//              of the adapter, not once per sequence -, runs the float32 chain over j ascending for the 16 rows (t from LDS as wave-wide
//              broadcasts) and lands one 4-byte read-modify-write per row at the gathered row.  LDS: 12 288 + 1 024 + 64 = 13 376 bytes.
//
// The LDS bound of the file: 18 496 bytes per workgroup.
#include "lora_common.h"
#include "lora_plan.h"

namespace {

struct Tile {
    int a;       // the adapter
    int rows;    // rows of the tile, 1 .. 16; 0: no such tile, leave
    int rank;    // the rank of the tile's first row among the adapter's rows
    int m0;      // the sequence of that row among the adapter's sequences: s_seq[0]
};

// The tile of workgroup blockIdx.x (the header comment has the steps).  s_cnt: int [LR_WAVES][64], s_seq: int [LR_TILE] of LDS.  Every
// thread of the workgroup calls it and gets the same answer; on return with rows > 0 s_seq is written and a barrier has passed.
__device__ __forceinline__ Tile find_tile(const int* __restrict__ ids, int S, int slots, int rps, int (*s_cnt)[64], int* s_seq) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int per = (S + LR_THREADS - 1) / LR_THREADS * 64;                  // sequences of a wave's quarter (a multiple of 64)
    const int s_begin = wave * per, s_end = s_begin + per < S ? s_begin + per : S;
    s_cnt[wave][lane] = 0;                                                   // (the wave's own row: its LDS operations stay in order)
    for (int s = s_begin + lane; s < s_end; s += 64) {
        const int id = ids[s];
        if ((unsigned)id < (unsigned)slots) atomicAdd(&s_cnt[wave][id], 1);
    }
    __syncthreads();
    // lane = adapter: its sequences in every quarter, its tiles, the inclusive prefix of the tiles
    int seqs = 0, before = 0, mine = 0;
#pragma unroll
    for (int w = 0; w < LR_WAVES; ++w) {
        const int c = s_cnt[w][lane];
        seqs += c;
        before += w < wave ? c : 0;
        mine = w == wave ? c : mine;
    }
    const int tiles = (seqs * rps + LR_TILE - 1) / LR_TILE;
    int incl = tiles;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int v = __shfl_up(incl, d);
        if (lane >= d) incl += v;
    }
    const int tile = blockIdx.x;
    const unsigned long long holds = __ballot(tile < incl);
    Tile t = {0, 0, 0, 0};
    if (holds == 0ull) return t;                                             // past the last real tile (workgroup-uniform)
    t.a = __ffsll((long long)holds) - 1;
    t.rank = (tile - __builtin_amdgcn_readfirstlane(__shfl(incl - tiles, t.a))) * LR_TILE;
    const int total = __builtin_amdgcn_readfirstlane(__shfl(seqs, t.a)) * rps;
    t.rows = total - t.rank < LR_TILE ? total - t.rank : LR_TILE;
    t.m0 = t.rank / rps;
    const int m1 = (t.rank + t.rows - 1) / rps;
    int run = __builtin_amdgcn_readfirstlane(__shfl(before, t.a));           // matches in the earlier quarters
    const int stop = run + __builtin_amdgcn_readfirstlane(__shfl(mine, t.a));
    if (run <= m1 && stop > t.m0) {                                          // this quarter holds sequences of the tile (wave-uniform)
        for (int s0 = s_begin; s0 < s_end && run <= m1; s0 += 64) {
            const int s = s0 + lane;
            const bool match = s < s_end && ids[s] == t.a;
            const unsigned long long mk = __ballot(match);
            const int m = run + __popcll(mk & ((1ull << lane) - 1ull));
            if (match && m >= t.m0 && m <= m1) s_seq[m - t.m0] = s;
            run += __popcll(mk);
        }
    }
    __syncthreads();
    return t;
}

// row i (< t.rows) of the tile, in the batch
__device__ __forceinline__ int tile_row(const Tile& t, const int* s_seq, int rps, int i) {
    const int rk = t.rank + i, m = rk / rps;
    return s_seq[m - t.m0] * rps + (rk - m * rps);
}

// A float32 value the compiler has to produce as such.  The rule's last step is fp16(fmaf(scaling, acc, float(old))): a float32 fma, then
// the rounding to fp16.  Left alone the compiler folds the two into v_fma_mixlo_f16 / v_fma_mixhi_f16 - ONE rounding, which differs
// from lora_rows.hip's two in about one element of 20 000 by an fp16 ulp.
__device__ __forceinline__ float as_f32(float v) {
    asm volatile("" : "+v"(v));
    return v;
}

// grid = (tile bound, K slices, j groups), 256 threads.  S = T / rps sequences; R = nseg * r.  The launcher checks everything.
__global__ __launch_bounds__(LR_THREADS) void lora_grouped_shrink_kernel(const int8_t* __restrict__ x, long long x_stride,
                                                                         const _Float16* __restrict__ A,
                                                                         const int* __restrict__ seq_adapter, int S, int slots, int K, int R,
                                                                         int rps, int T, float* __restrict__ ws) {
    __shared__ __attribute__((aligned(16))) float s_red[LR_WAVES][LR_TILE][LR_RED_LD];
    __shared__ int s_cnt[LR_WAVES][64];
    __shared__ int s_seq[LR_TILE];
    const Tile tl = find_tile(seq_adapter, S, slots, rps, s_cnt, s_seq);
    if (tl.rows == 0) return;
    const int a = tl.a, rows = tl.rows;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
    const int j0 = blockIdx.z * LR_JGROUP;
    const int k0 = blockIdx.y * LR_KSLICE + wave * (LR_KSLICE / LR_WAVES);
    v4f acc[4];
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) acc[jt] = v4f{0.f, 0.f, 0.f, 0.f};
    if (k0 < K) {                                        // (wave-uniform; K is a multiple of 128: a wave's range is whole or absent)
        h8 xb[4];
        const int8_t* xp = x + (size_t)(c < rows ? tile_row(tl, s_seq, rps, c) : 0) * x_stride + k0 + 8 * g;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            v2u raw = {0u, 0u};
            if (c < rows) raw = *reinterpret_cast<const v2u*>(xp + 32 * ks);
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
        *reinterpret_cast<v4f*>(ws + ((size_t)blockIdx.y * T + tile_row(tl, s_seq, rps, t)) * R + j0 + jq) = sum;
    }
}

// grid = (tile bound, ysplit <= N slices), 256 threads.  e0, e1: the ends of segments 0 and 1 (INT_MAX where there is no such boundary).
__global__ __launch_bounds__(LR_THREADS) void lora_grouped_expand_kernel(_Float16* __restrict__ out, long long out_stride,
                                                                         const _Float16* __restrict__ x_scale,
                                                                         const _Float16* __restrict__ B, const float* __restrict__ scaling,
                                                                         const int* __restrict__ seq_adapter, int S, int slots, int N, int r,
                                                                         int R, int rps, int T, int kslices, int e0, int e1,
                                                                         const float* __restrict__ ws) {
    __shared__ __attribute__((aligned(16))) float s_t[LR_TILE][LR_MAX_R];
    __shared__ int s_cnt[LR_WAVES][64];
    __shared__ int s_seq[LR_TILE];
    const Tile tl = find_tile(seq_adapter, S, slots, rps, s_cnt, s_seq);
    if (tl.rows == 0) return;
    const int a = tl.a, rows = tl.rows, tid = threadIdx.x;
    const int nslices = (N + LR_NSLICE - 1) / LR_NSLICE;
    _Float16* op[LR_TILE];                               // the tile's rows of out (workgroup-uniform)
#pragma unroll
    for (int t = 0; t < LR_TILE; ++t) op[t] = out + (size_t)(t < rows ? tile_row(tl, s_seq, rps, t) : 0) * out_stride;

    // what does not depend on the planes is requested first, so that its latency runs beside the staging: the thread's rows of `out`
    // and the first 8 rank columns of its two rows of B, for the first column slice
    int ns = blockIdx.y;
    int n = ns * LR_NSLICE + 2 * tid;
    bool mine = n < N;
    const _Float16* __restrict__ bp = B + ((size_t)a * N + (mine ? n : 0)) * r;
    u32 o[LR_TILE];
    h8 b0 = {}, b1 = {};
    auto request = [&]() {
#pragma unroll
        for (int t = 0; t < LR_TILE; ++t) {
            o[t] = 0u;
            if (mine && t < rows) o[t] = *reinterpret_cast<const u32*>(op[t] + n);
        }
        if (mine) {
            b0 = *reinterpret_cast<const h8*>(bp);
            b1 = *reinterpret_cast<const h8*>(bp + r);
        }
    };
    request();

    // ---- 1. t[row, j] = x_scale[row] * (the K-slice planes summed in slice order), all segments
    const int q = R >> 2;
    for (int i = tid; i < rows * q; i += LR_THREADS) {
        const int t = i / q, j4 = (i - t * q) * 4, row = tile_row(tl, s_seq, rps, t);
        const float* p = ws + (size_t)row * R + j4;
        v4f sum = *reinterpret_cast<const v4f*>(p);
#pragma unroll 8
        for (int sl = 1; sl < kslices; ++sl) sum += *reinterpret_cast<const v4f*>(p + (size_t)sl * T * R);
        const float sx = (float)x_scale[row];
        *reinterpret_cast<v4f*>(&s_t[t][j4]) = sum * sx;
    }
    __syncthreads();

    // ---- 2. two columns per thread, every row of the tile, one column slice after the other (no barrier from here on)
    const float sc = scaling[a];
    for (;;) {
        if (mine) {
            const int seg = (n >= e0 ? 1 : 0) + (n >= e1 ? 1 : 0);
            float acc0[LR_TILE], acc1[LR_TILE];
#pragma unroll
            for (int t = 0; t < LR_TILE; ++t) acc0[t] = acc1[t] = 0.f;
            for (int j0 = 0; j0 < r; j0 += 8) {
                h8 nb0 = b0, nb1 = b1;
                if (j0 + 8 < r) {                        // the next 8 rank columns, requested before this chunk's arithmetic
                    nb0 = *reinterpret_cast<const h8*>(bp + j0 + 8);
                    nb1 = *reinterpret_cast<const h8*>(bp + r + j0 + 8);
                }
                const float* sp = &s_t[0][seg * r + j0];
#pragma unroll
                for (int t = 0; t < LR_TILE; ++t) {
                    if (t < rows) {                      // (workgroup-uniform)
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
                    const float y0 = as_f32(__builtin_fmaf(sc, acc0[t], (float)old[0])), y1 = as_f32(__builtin_fmaf(sc, acc1[t], (float)old[1]));
                    *reinterpret_cast<u32*>(op[t] + n) = pack_h2(y0, y1);
                }
            }
        }
        ns += gridDim.y;
        if (ns >= nslices) break;                        // (workgroup-uniform)
        n = ns * LR_NSLICE + 2 * tid;
        mine = n < N;
        bp = B + ((size_t)a * N + (mine ? n : 0)) * r;
        request();
    }
}

}  // namespace

extern "C" int qs_lora_rows_form(int T, int rows_per_seq, int slots) {
    QS_REQUIRE(T >= 0 && T <= LR_MAX_ROWS && rows_per_seq >= 1 && T % rows_per_seq == 0 && slots >= 1,
               "lora_rows_form: T=%d (0 .. %d) must be a multiple of rows_per_seq=%d (>= 1), slots=%d (>= 1)", T, LR_MAX_ROWS, rows_per_seq, slots);
    return (int)lora_plan::lora_form(T, rows_per_seq, slots);
}

extern "C" int qs_lora_rows_grouped_tiles(int T, int rows_per_seq, int slots) {
    QS_REQUIRE(T >= 0 && T <= LR_MAX_ROWS && rows_per_seq >= 1 && T % rows_per_seq == 0 && slots >= 1,
               "lora_rows_grouped_tiles: T=%d (0 .. %d) must be a multiple of rows_per_seq=%d (>= 1), slots=%d (>= 1)", T, LR_MAX_ROWS,
               rows_per_seq, slots);
    return lora_plan::grouped_tiles(T, rows_per_seq, slots);
}

extern "C" int qs_lora_rows_grouped(void* out, int64_t out_stride, const int8_t* x, int64_t x_stride, const void* x_scale, const void* A,
                                    const void* B, const float* scaling, const int32_t* seq_adapter, int slots, int T, int K, int N, int r,
                                    int rows_per_seq, int nseg, int seg_end0, int seg_end1, int seg_end2, void* workspace,
                                    int64_t workspace_size, qs_stream_t stream) {
    const int ends[LR_MAX_SEG] = {seg_end0, seg_end1, seg_end2};
    int rc = lora_check_args("lora_rows_grouped", out, out_stride, x, x_stride, x_scale, A, B, scaling, seq_adapter, slots, T, K, N, r,
                             rows_per_seq, nseg, ends, workspace, workspace_size);
    if (rc != QS_OK) return rc;
    const char* why = lora_plan::grouped_refusal(T, rows_per_seq, slots);
    QS_REQUIRE(!why, "lora_rows_grouped: T=%d, rows_per_seq=%d, slots=%d: %s", T, rows_per_seq, slots, why);
    if (T == 0) return QS_OK;
    const int R = nseg * r, S = T / rows_per_seq, tiles = lora_plan::grouped_tiles(T, rows_per_seq, slots);
    const int kslices = (K + LR_KSLICE - 1) / LR_KSLICE, nslices = (N + LR_NSLICE - 1) / LR_NSLICE;
    const int e0 = nseg >= 2 ? ends[0] : INT32_MAX, e1 = nseg >= 3 ? ends[1] : INT32_MAX;
    hipLaunchKernelGGL(lora_grouped_shrink_kernel, dim3(tiles, kslices, (R + LR_JGROUP - 1) / LR_JGROUP), dim3(LR_THREADS), 0,
                       (hipStream_t)stream, x, (long long)x_stride, (const _Float16*)A, seq_adapter, S, slots, K, R, rows_per_seq, T,
                       (float*)workspace);
    rc = qs_launch_status("lora_rows_grouped (shrink)");
    if (rc != QS_OK) return rc;
    hipLaunchKernelGGL(lora_grouped_expand_kernel, dim3(tiles, lora_plan::grouped_expand_ysplit(tiles, nslices)), dim3(LR_THREADS), 0,
                       (hipStream_t)stream, (_Float16*)out, (long long)out_stride, (const _Float16*)x_scale, (const _Float16*)B, scaling,
                       seq_adapter, S, slots, N, r, R, rows_per_seq, T, kslices, e0, e1, (const float*)workspace);
    return qs_launch_status("lora_rows_grouped (expand)");
}
