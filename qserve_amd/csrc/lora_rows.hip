// lora_rows.hip -- multi-LoRA next to the W4A8 linears, for MI355X (gfx950): out[t, :] += scaling[a] * B[a] (A[a] x[t]) with a = the adapter
// of row t's SEQUENCE, on the int8 activations the base GEMM of the same linear read.  DESIGN.md 10 ("LoRA adapters", "Grouped rows"); the
// rule is the header comment of qs_lora_rows in include/qserve_amd.h.  Rows are sequence-major with rows_per_seq rows per sequence.  A
// workgroup works on a TILE of up to 16 rows under ONE adapter - it reads a slice of A or B once for the whole tile - and the file
// holds the two forms that differ in what a tile is:
//
//   the ROWS form (qs_lora_rows): up to 16 consecutive rows of one sequence, ceil(rows_per_seq / 16) tiles per sequence; the adapter is
//              one read of seq_adapter.  A tile whose id is outside 0 .. slots-1 leaves both kernels at once.
//   the GROUPED form (qs_lora_rows_grouped; GroupedTile): 16 rows of one ADAPTER, wherever they sit in the batch.  The rows of adapter a
//              are all rows t with seq_adapter[t / rows_per_seq] == a in ascending t; tile i of adapter a is rows 16 i .. 16 i + 15 of
//              that list; the tiles of adapter 0 come first in the grid, then those of adapter 1 ...  At rows_per_seq < 16 the rows
//              form's tiles are mostly padding and A / B are fetched again for every sequence; here every column of the MFMA is a real
//              row and a slice of A or B is read once per 16 rows of its adapter.  Rows of an id outside 0 .. slots-1 belong to no tile.
//
// Under either form nothing of a row without an adapter is read or written and no address is formed from its id.  The workspace is the
// same (qs_lora_rows_workspace: float32 K-slice planes [K slices, T, nseg * r], indexed by the ORIGINAL row; no permutation is stored).
// No atomic decides an order, no cross-workgroup wait inside a launch, no scratch; every sum has a fixed order, stated once in front of
// the kernels, so results are bit-identical run to run, eager against graph replay, and between the forms: the form is a choice of
// cost alone (lora_plan.h), and tests/golden/lora_bits.json pins the bits of every form.
//
// The two forms share one translation unit, one flag setting (build.py: the default one), the staging and landing steps and the host
// prologue of lora_common.h - but NOT one kernel body.  One shrink body and one expand body over a tile type (row(i) = row0 + i against
// GroupedTile) were built and measured (profiles/lora_one_body.txt): the same bits, the grouped form at the same speed, the rows form
// 5 - 27 % slower wherever a tile has few rows (one row per sequence: the decode step) - the grouped expand's list of 16 row pointers in
// front of its first load alone costs a one-row tile 20 % at gate_up, and without it the call still lost 4 - 10 % at down (K = 14 336).
// So the rows form keeps its own two kernels, which form their addresses where they use them.  Smaller shares were measured too and are
// not in either: the MFMA chains, the wave-order sum and the float32 chains as device functions called by all four kernels cost both
// forms up to 8 % (down and gate_up at r = 64); the rows kernels on SeqTile and lora_stage alone cost the rows form 1 % in the median,
// 3 - 6 % on the lines of a decode step that leaves at once.
//
// A grouped workgroup FINDS ITS OWN TILE on the device (GroupedTile; nothing of the ids reaches the host, so a captured graph follows
// ids changed in place).  The grid's tile extent is lora_plan.h's bound ceil(T / 16) + min(slots, S) - 1, S = T / rows_per_seq
// sequences; a workgroup past the last real tile leaves at once.  The scan reads the S ids, not the T rows: wave w counts the ids of
// ITS contiguous quarter of the sequences per adapter into its own row of LDS counters (integer adds: a count has no order); after one
// barrier every wave adds the four rows per adapter (lane = adapter), turns rows into tiles, takes an inclusive prefix over the lanes
// and picks with one ballot the adapter whose tile range holds blockIdx.x - that gives (adapter, first rank); the wave whose quarter
// holds sequences of that rank range walks it again, 64 ids per round, and a ballot prefix over the matches, continued from the
// counts of the earlier quarters, places match number m at s_seq[m - first match] - ascending, so membership is deterministic; a
// second barrier, and row i of the tile is s_seq[(rank + i) / rows_per_seq - first match] * rows_per_seq + (rank + i) % rows_per_seq.
//
// This file holds FOUR kernels:
//
//   lora_shrink_kernel
//   lora_grouped_shrink_kernel
//              grid = (tiles, K slices of 512, groups of 64 rank rows), 256 threads; the grouped form's tile extent is lora_plan.h's tile
//              bound.  t[j, row] = sum_k A[a, j, k] x[row, k] on v_mfma_f32_16x16x32_f16: the M index is the rank row j (A operand: 16
//              bytes of A per lane, straight from memory), the N index the tile's row (B operand: 8 int8 of x per lane at the tile's row,
//              converted to fp16 - exact), so a result register holds four consecutive j of one row.  Wave w takes k in [128 w, 128 w +
//              128) of the slice (four k-steps, all loads issued up front) for up to four 16-row j tiles; the four waves' results meet in
//              LDS (rows padded to 68 floats: the 16-byte stores of a wave fall on distinct banks) and are summed in wave order into the
//              workspace plane of the K slice at the tile's row.  One workgroup per (tile, 512-slice) and NOT per (tile, 128-chunk): the
//              chunk sums of a slice have to be added in chunk order before they land in the slice's plane; workgroups per chunk would
//              need a plane per chunk - four times the workspace the contract fixes - or an ordered hand-over between workgroups, which
//              is ruled out.  So the finer split was not built; few-tile calls fill the CUs through the K slices and rank groups
//              (profiles/lora_grouped.txt).  LDS: 17 408 bytes; grouped 17 408 + 1 024 (counters) + 64 (sequences) = 18 496.
//
//   lora_expand_kernel
//   lora_grouped_expand_kernel
//              grid = (tiles, N slices of 512), 256 threads, two adjacent output columns per thread; the grouped form's grid is (tile
//              bound, ysplit).  The thread's rows of out and its first 8 rank columns of B for the workgroup's (first) column slice are
//              requested; the tile's t[row, j] = x_scale[row] * (the K-slice planes summed in slice order) is staged in LDS, all segments
//              (at most 16 x 192 floats), their latency runs beside the staging; then every thread takes the r values of B for each of
//              its two columns, 8 at a time - read once per tile -, runs the float32 chain over j ascending for every row of the tile (t
//              from LDS as wave-wide broadcasts; the segment g is that of the thread's own columns: segment ends are multiples of 64, a
//              pair never straddles one) and lands one 4-byte read-modify-write per row at the tile's row.  The rows form's grid has a
//              workgroup for every slice; a grouped workgroup walks the slices blockIdx.y, blockIdx.y + ysplit, ... (lora_plan.h: with
//              many tiles it keeps its tile for several slices, so the id scan and the staging are paid once for them).  LDS: 12 288
//              bytes; grouped 12 288 + 1 024 + 64 = 13 376.
//
// The LDS bound of the file: 18 496 bytes per workgroup.
#include "lora_common.h"
#include "lora_plan.h"

namespace {

// The tile of workgroup blockIdx.x of the grouped form (the header comment has the steps).  s_cnt: int [LR_WAVES][64], s_seq: int
// [LR_TILE] of LDS.  Every thread of the workgroup constructs it and gets the same answer; with rows > 0 s_seq is written and a barrier
// has passed.
struct GroupedTile {
    int a;       // the adapter
    int rows;    // rows of the tile, 1 .. 16; 0: no such tile, leave
    int rank;    // the rank of the tile's first row among the adapter's rows
    int m0;      // the sequence of that row among the adapter's sequences: s_seq[0]
    int rps;
    const int* s_seq;
    __device__ __forceinline__ GroupedTile(const int* __restrict__ ids, int S, int slots, int rps_, int (*s_cnt)[64], int* s_seq_)
        : a(0), rows(0), rank(0), m0(0), rps(rps_), s_seq(s_seq_) {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const int per = (S + LR_THREADS - 1) / LR_THREADS * 64;              // sequences of a wave's quarter (a multiple of 64)
        const int s_begin = wave * per, s_end = s_begin + per < S ? s_begin + per : S;
        s_cnt[wave][lane] = 0;                                               // (the wave's own row: its LDS operations stay in order)
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
        if (holds == 0ull) return;                                           // past the last real tile (workgroup-uniform)
        a = __ffsll((long long)holds) - 1;
        rank = (tile - __builtin_amdgcn_readfirstlane(__shfl(incl - tiles, a))) * LR_TILE;
        const int total = __builtin_amdgcn_readfirstlane(__shfl(seqs, a)) * rps;
        rows = total - rank < LR_TILE ? total - rank : LR_TILE;
        m0 = rank / rps;
        const int m1 = (rank + rows - 1) / rps;
        int run = __builtin_amdgcn_readfirstlane(__shfl(before, a));         // matches in the earlier quarters
        const int stop = run + __builtin_amdgcn_readfirstlane(__shfl(mine, a));
        if (run <= m1 && stop > m0) {                                        // this quarter holds sequences of the tile (wave-uniform)
            for (int s0 = s_begin; s0 < s_end && run <= m1; s0 += 64) {
                const int s = s0 + lane;
                const bool match = s < s_end && ids[s] == a;
                const unsigned long long mk = __ballot(match);
                const int m = run + __popcll(mk & ((1ull << lane) - 1ull));
                if (match && m >= m0 && m <= m1) s_seq_[m - m0] = s;
                run += __popcll(mk);
            }
        }
        __syncthreads();
    }
    // row i (< rows) of the tile, in the batch
    __device__ __forceinline__ int row(int i) const {
        const int rk = rank + i, m = rk / rps;
        return s_seq[m - m0] * rps + (rk - m * rps);
    }
};

// THE ORDER OF EVERY SUM, in the four kernels below - what all forms, the prompt form of lora_prompt.hip included, reproduce bit for bit:
// per row and rank row a chain of four MFMA k-steps over each 128-chunk of K from +0.0 (fp16 x fp16 products are exact in float32; only
// the float32 additions round; an absent chunk of a partial last slice is the idle wave's +0.0); the four chunk sums of a 512-slice
// added in chunk order (= wave order); the slices added in slice order; one multiply by float(x_scale) (lora_stage does both in the
// grouped and the prompt form); acc = fmaf(float(B[n, j]), t_j, acc) over j ascending from +0.0; fp16(fmaf(scaling, acc, float(old)))
// (lora_land, in every form).  An MFMA column depends on its own operand column only, so which rows share a tile does not change a
// row's value.  Every float32 step is an explicit operation - an add or a multiply alone, or __builtin_fmaf -, nothing the compiler
// may contract in one kernel and not in another.

// ---- the rows form
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
            *reinterpret_cast<u32*>(out + (size_t)(row0 + t) * out_stride + n) = lora_land(o[t], sc, acc0[t], acc1[t]);
        }
    }
}

// ---- the grouped form: the same two kernels behind GroupedTile, the rows gathered through tl.row; the expand walks column slices.
// S = T / rps sequences.
__global__ __launch_bounds__(LR_THREADS) void lora_grouped_shrink_kernel(const int8_t* __restrict__ x, long long x_stride,
                                                                         const _Float16* __restrict__ A,
                                                                         const int* __restrict__ seq_adapter, int S, int slots, int K, int R,
                                                                         int rps, int T, float* __restrict__ ws) {
    __shared__ __attribute__((aligned(16))) float s_red[LR_WAVES][LR_TILE][LR_RED_LD];
    __shared__ int s_cnt[LR_WAVES][64];
    __shared__ int s_seq[LR_TILE];
    const GroupedTile tl(seq_adapter, S, slots, rps, s_cnt, s_seq);
    if (tl.rows == 0) return;                            // past the last real tile (workgroup-uniform)
    const int a = tl.a, rows = tl.rows;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
    const int j0 = blockIdx.z * LR_JGROUP;
    const int k0 = blockIdx.y * LR_KSLICE + wave * (LR_KSLICE / LR_WAVES);
    v4f acc[4];
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) acc[jt] = v4f{0.f, 0.f, 0.f, 0.f};
    if (k0 < K) {                                        // (wave-uniform; K is a multiple of 128: a wave's range is whole or absent)
        h8 xb[4];
        const int8_t* xp = x + (size_t)(c < rows ? tl.row(c) : 0) * x_stride + k0 + 8 * g;
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
        *reinterpret_cast<v4f*>(ws + ((size_t)blockIdx.y * T + tl.row(t)) * R + j0 + jq) = sum;
    }
}

__global__ __launch_bounds__(LR_THREADS) void lora_grouped_expand_kernel(_Float16* __restrict__ out, long long out_stride,
                                                                         const _Float16* __restrict__ x_scale,
                                                                         const _Float16* __restrict__ B, const float* __restrict__ scaling,
                                                                         const int* __restrict__ seq_adapter, int S, int slots, int N, int r,
                                                                         int R, int rps, int T, int kslices, int e0, int e1,
                                                                         const float* __restrict__ ws) {
    __shared__ __attribute__((aligned(16))) float s_t[LR_TILE][LR_MAX_R];
    __shared__ int s_cnt[LR_WAVES][64];
    __shared__ int s_seq[LR_TILE];
    const GroupedTile tl(seq_adapter, S, slots, rps, s_cnt, s_seq);
    if (tl.rows == 0) return;                            // past the last real tile (workgroup-uniform)
    const int a = tl.a, rows = tl.rows, tid = threadIdx.x;
    const int nslices = (N + LR_NSLICE - 1) / LR_NSLICE;
    _Float16* op[LR_TILE];                               // the tile's rows of out (workgroup-uniform)
#pragma unroll
    for (int t = 0; t < LR_TILE; ++t) op[t] = out + (size_t)(t < rows ? tl.row(t) : 0) * out_stride;

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
    lora_stage(&s_t[0][0], LR_MAX_R, tl, R, T, kslices, ws, x_scale);
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
            for (int t = 0; t < LR_TILE; ++t)
                if (t < rows) *reinterpret_cast<u32*>(op[t] + n) = lora_land(o[t], sc, acc0[t], acc1[t]);
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

extern "C" int64_t qs_lora_rows_workspace(int T, int K, int r, int nseg) {
    QS_REQUIRE(T >= 0 && T <= LR_MAX_ROWS && K >= 128 && K <= LR_MAX_K && K % 128 == 0 && rank_ok(r) && nseg >= 1 && nseg <= LR_MAX_SEG,
               "lora_rows_workspace: T=%d (0 .. %d), K=%d (a multiple of 128, <= %d), r=%d (8, 16, 32, 64), nseg=%d (1 .. 3)", T,
               LR_MAX_ROWS, K, LR_MAX_K, r, nseg);
    return workspace_bytes(T, K, r, nseg);
}

// ---- the planner's entry points (lora_plan.h), of all three forms
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

extern "C" int qs_lora_rows_prompt_run(int tiles, int kslices) {
    QS_REQUIRE(tiles >= 1 && kslices >= 1, "lora_rows_prompt_run: tiles=%d, K slices=%d (>= 1)", tiles, kslices);
    return lora_plan::prompt_run(tiles, kslices);
}

extern "C" int qs_lora_rows_form_for_rank(int form, int r) {
    QS_REQUIRE(form >= 0 && form <= (int)lora_plan::LORA_PROMPT && rank_ok(r), "lora_rows_form_for_rank: form=%d (0 .. 2), r=%d (8, 16, 32 or 64)", form, r);
    return (int)lora_plan::planned_for_rank((lora_plan::LoraForm)form, r);
}

// ---- the two 16-row forms
extern "C" int qs_lora_rows(void* out, int64_t out_stride, const int8_t* x, int64_t x_stride, const void* x_scale, const void* A,
                            const void* B, const float* scaling, const int32_t* seq_adapter, int slots, int T, int K, int N, int r,
                            int rows_per_seq, int nseg, int seg_end0, int seg_end1, int seg_end2, void* workspace, int64_t workspace_size,
                            qs_stream_t stream) {
    LoraCall c;
    int rc = lora_prologue("lora_rows", c, out, out_stride, x, x_stride, x_scale, A, B, scaling, seq_adapter, slots, T, K, N, r, rows_per_seq,
                           nseg, seg_end0, seg_end1, seg_end2, workspace, workspace_size);
    if (rc != QS_OK) return rc;
    if (T == 0) return QS_OK;
    const int tps = (rows_per_seq + LR_TILE - 1) / LR_TILE, tiles = T / rows_per_seq * tps;
    hipLaunchKernelGGL(lora_shrink_kernel, dim3(tiles, c.kslices, (c.R + LR_JGROUP - 1) / LR_JGROUP), dim3(LR_THREADS), 0, (hipStream_t)stream,
                       x, (long long)x_stride, c.A, seq_adapter, slots, K, c.R, rows_per_seq, tps, T, c.ws);
    rc = qs_launch_status("lora_rows (shrink)");
    if (rc != QS_OK) return rc;
    hipLaunchKernelGGL(lora_expand_kernel, dim3(tiles, c.nslices), dim3(LR_THREADS), 0, (hipStream_t)stream, c.out, (long long)out_stride,
                       c.x_scale, c.B, scaling, seq_adapter, slots, N, r, c.R, rows_per_seq, tps, T, c.kslices, c.e0, c.e1, c.ws);
    return qs_launch_status("lora_rows (expand)");
}

extern "C" int qs_lora_rows_grouped(void* out, int64_t out_stride, const int8_t* x, int64_t x_stride, const void* x_scale, const void* A,
                                    const void* B, const float* scaling, const int32_t* seq_adapter, int slots, int T, int K, int N, int r,
                                    int rows_per_seq, int nseg, int seg_end0, int seg_end1, int seg_end2, void* workspace,
                                    int64_t workspace_size, qs_stream_t stream) {
    LoraCall c;
    int rc = lora_prologue("lora_rows_grouped", c, out, out_stride, x, x_stride, x_scale, A, B, scaling, seq_adapter, slots, T, K, N, r,
                           rows_per_seq, nseg, seg_end0, seg_end1, seg_end2, workspace, workspace_size);
    if (rc != QS_OK) return rc;
    const char* why = lora_plan::grouped_refusal(T, rows_per_seq, slots);
    QS_REQUIRE(!why, "lora_rows_grouped: T=%d, rows_per_seq=%d, slots=%d: %s", T, rows_per_seq, slots, why);
    if (T == 0) return QS_OK;
    const int S = T / rows_per_seq, tiles = lora_plan::grouped_tiles(T, rows_per_seq, slots);
    hipLaunchKernelGGL(lora_grouped_shrink_kernel, dim3(tiles, c.kslices, (c.R + LR_JGROUP - 1) / LR_JGROUP), dim3(LR_THREADS), 0,
                       (hipStream_t)stream, x, (long long)x_stride, c.A, seq_adapter, S, slots, K, c.R, rows_per_seq, T, c.ws);
    rc = qs_launch_status("lora_rows_grouped (shrink)");
    if (rc != QS_OK) return rc;
    hipLaunchKernelGGL(lora_grouped_expand_kernel, dim3(tiles, lora_plan::grouped_expand_ysplit(tiles, c.nslices)), dim3(LR_THREADS), 0,
                       (hipStream_t)stream, c.out, (long long)out_stride, c.x_scale, c.B, scaling, seq_adapter, S, slots, N, r, c.R,
                       rows_per_seq, T, c.kslices, c.e0, c.e1, c.ws);
    return qs_launch_status("lora_rows_grouped (expand)");
}
