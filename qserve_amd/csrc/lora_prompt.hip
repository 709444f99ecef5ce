// lora_prompt.hip -- the PROMPT form of the multi-LoRA row update of lora_rows.hip, for MI355X (gfx950): the same rule (qs_lora_rows in
// include/qserve_amd.h), the same bits, but a TILE is up to 64 consecutive rows of one SEQUENCE, not 16: ceil(rows_per_seq / 64) tiles per
// sequence, the last one short.  DESIGN.md 10 ("Prompt tiles").  For the passes with many rows per sequence - prefill, prefill_chunked,
// a wide verify_tree -, where a 16-row tile fetches a slice of A or B again for every 16 rows, ends every shrink workgroup in a
// cross-wave LDS exchange behind a barrier and makes the grid as large as the row count.  A tile whose adapter is outside 0 .. slots-1
// leaves both kernels at once: nothing of its rows is read or written, no address is formed from the id.  The id is read on the
// device, so a captured call follows ids changed in place.  The workspace is exactly the rows form's (qs_lora_rows_workspace: float32
// K-slice planes [K slices, T, nseg * r]).
//
// Every sum runs in the order lora_rows.hip states in front of its kernels, the staging and the landing step are lora_common.h's, shared
// with the 16-row forms.  An MFMA column depends on its own operand column only and an MFMA row on its own operand row only, so which
// rows share a tile - and what stands in the columns and rows nobody stores - does not change a value.  No atomics, no cross-workgroup
// wait inside a launch, no scratch.  This file holds TWO kernels:
//
//   lora_prompt_shrink_kernel<NJT>   grid = (tiles, runs of K slices, rank groups of 16 NJT <= 64 rank rows), 256 threads, NO LDS and NO
//              barrier.  Wave w owns rows 16 w .. 16 w + 15 of the tile - a wave whose block is empty leaves - and whole 512-slices:
//              for a slice it runs the four chunk chains on v_mfma_f32_16x16x32_f16 in its own registers (M the rank row, A 16 bytes
//              per lane straight from memory; N the row, 8 int8 of x per lane, int8 -> fp16 exactly) for its NJT rank tiles, adds them
//              in chunk order and writes the slice's plane at its rows straight from the result registers (16 bytes per lane).  A
//              workgroup walks the lora_plan.h run of consecutive slices; the operands of chunk q + 1 are requested before the
//              arithmetic of chunk q.  Lanes of rows past the tile's end and of rank rows past R read a clamped, valid address: their
//              MFMA columns / rows are never stored.  The four waves read the same lines of A 16 bytes per lane, as the rows form
//              does: the LDS fill of A (one fetch per workgroup) was NOT built and the two were not compared.
//
//   lora_prompt_expand_kernel<RK>   grid = (tiles, ysplit), 256 threads, two adjacent output columns per thread, r = RK.  The tile's
//              t[row, j] = x_scale[row] * (the K-slice planes summed in slice order) is staged in LDS for its up to 64 rows, all
//              segments (64 x R floats, dynamic: 49 152 bytes at R = 192); the first block's rows of out and B are requested before.
//              Then the workgroup walks the column slices blockIdx.y, blockIdx.y + ysplit, ... of 512 columns: a thread holds ALL r
//              values of B for its two columns in registers - read once per 64 rows of the sequence -, walks the tile's 16-row
//              blocks with the float32 chain over j ascending (four rows and 8 rank columns a step, t from LDS as wave-wide broadcasts
//              requested one step ahead), requests the next block's rows of out before the current block's arithmetic and lands one
//              4-byte read-modify-write per row.  A short last block runs
//              the chain on LDS rows nobody staged and stores nothing of them.  Four columns per thread were not built.
//
// The LDS bound of the file: 49 152 bytes per workgroup (the expand at R = 192; the shrink uses none).
#include "lora_common.h"
#include "lora_plan.h"

namespace {

constexpr int LP_TILE = lora_plan::PROMPT_TILE;      // rows per workgroup: one MFMA block of LR_TILE rows per wave
static_assert(LP_TILE == LR_WAVES * LR_TILE, "a wave owns one 16-row block of the tile");

using PromptTile = SeqTile<LP_TILE>;

// the operands of one 128-chunk of K in a lane: 8 int8 of x and 8 fp16 of A per rank tile, for each of the four k-steps
template <int NJT>
struct ChunkOps {
    v2u xr[4];
    v4u ar[NJT][4];
};

template <int NJT>
__device__ __forceinline__ void request(ChunkOps<NJT>& o, const int8_t* xp, const _Float16* (&ap)[NJT], int k0) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) o.xr[ks] = *reinterpret_cast<const v2u*>(xp + k0 + 32 * ks);
#pragma unroll
    for (int jt = 0; jt < NJT; ++jt)
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) o.ar[jt][ks] = *reinterpret_cast<const v4u*>(ap[jt] + k0 + 32 * ks);
}

// grid = (tiles, runs, rank groups), 256 threads.  tps: tiles per sequence; R = nseg * r; run: K slices per workgroup.  The launcher
// checks everything.
template <int NJT>
__global__ __launch_bounds__(LR_THREADS) void lora_prompt_shrink_kernel(const int8_t* __restrict__ x, long long x_stride,
                                                                        const _Float16* __restrict__ A, const int* __restrict__ seq_adapter,
                                                                        int slots, int K, int R, int rps, int tps, int T, int run,
                                                                        float* __restrict__ ws) {
    const PromptTile tl(seq_adapter, slots, rps, tps);
    if (tl.rows == 0) return;                            // the base model (workgroup-uniform)
    const int a = tl.a, rows = tl.rows;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
    if (wave * LR_TILE >= rows) return;                  // the wave's block is empty (no barrier in this kernel)
    const bool live = wave * LR_TILE + c < rows;
    const size_t row = tl.row(live ? wave * LR_TILE + c : 0);
    const int j0 = blockIdx.z * (16 * NJT);
    const int8_t* xp = x + row * x_stride + 8 * g;
    const _Float16* ap[NJT];
#pragma unroll
    for (int jt = 0; jt < NJT; ++jt) {
        const int j = j0 + 16 * jt + c;
        ap[jt] = A + ((size_t)a * R + (j < R ? j : R - 1)) * K + 8 * g;
    }
    const int kchunks = K >> 7, kslices = (K + LR_KSLICE - 1) / LR_KSLICE;
    const int sl0 = blockIdx.y * run, sl1 = sl0 + run < kslices ? sl0 + run : kslices;
    const int qend = 4 * sl1 < kchunks ? 4 * sl1 : kchunks;

    ChunkOps<NJT> nxt;
    request(nxt, xp, ap, 4 * sl0 * 128);                 // (sl0 < kslices: the slice's first chunk exists)
    for (int sl = sl0; sl < sl1; ++sl) {
        v4f sum[NJT];
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) {
            const int q = 4 * sl + ch;
            v4f acc[NJT];
#pragma unroll
            for (int jt = 0; jt < NJT; ++jt) acc[jt] = v4f{0.f, 0.f, 0.f, 0.f};
            if (q < kchunks) {                           // (workgroup-uniform; only the last slice of K may be partial)
                const ChunkOps<NJT> cur = nxt;
                if (q + 1 < qend) request(nxt, xp, ap, (q + 1) * 128);   // the next chunk, requested before this chunk's arithmetic
                h8 xb[4];
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) xb[ks] = s8_to_h8(cur.xr[ks]);
#pragma unroll
                for (int ks = 0; ks < 4; ++ks)           // NJT independent chains side by side, each in k-step order
#pragma unroll
                    for (int jt = 0; jt < NJT; ++jt)
                        acc[jt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, cur.ar[jt][ks]), xb[ks], acc[jt], 0, 0, 0);
            }
#pragma unroll
            for (int jt = 0; jt < NJT; ++jt) sum[jt] = ch == 0 ? acc[jt] : sum[jt] + acc[jt];
        }
        // a result register: the wave's row c, rank rows j0 + 16 jt + 4 g .. + 3 (R is a multiple of 8: four values are inside or
        // outside together)
        float* wp = ws + ((size_t)sl * T + row) * R + j0 + 4 * g;
#pragma unroll
        for (int jt = 0; jt < NJT; ++jt)
            if (live && j0 + 16 * jt + 4 * g < R) *reinterpret_cast<v4f*>(wp + 16 * jt) = sum[jt];
    }
}

// grid = (tiles, ysplit <= N slices), 256 threads, 64 * R floats of dynamic LDS.  e0, e1: the ends of segments 0 and 1 (INT_MAX where
// there is no such boundary).
template <int RK>
__global__ __launch_bounds__(LR_THREADS) void lora_prompt_expand_kernel(_Float16* __restrict__ out, long long out_stride,
                                                                        const _Float16* __restrict__ x_scale, const _Float16* __restrict__ B,
                                                                        const float* __restrict__ scaling, const int* __restrict__ seq_adapter,
                                                                        int slots, int N, int R, int rps, int tps, int T, int kslices, int e0,
                                                                        int e1, const float* __restrict__ ws) {
    extern __shared__ __attribute__((aligned(16))) float s_t[];   // [LP_TILE][R]
    const PromptTile tl(seq_adapter, slots, rps, tps);
    if (tl.rows == 0) return;                            // the base model (workgroup-uniform)
    const int a = tl.a, rows = tl.rows, tid = threadIdx.x;
    const size_t row0 = tl.row0;
    const int nslices = (N + LR_NSLICE - 1) / LR_NSLICE;

    // the thread's columns of the current column slice, and block `blk` of the tile's rows of out for them.  Loads take no branch: a
    // thread past N reads the slice's last pair of columns, a row past the tile's end reads the tile's last row; neither is stored.
    int ns = blockIdx.y, n = ns * LR_NSLICE + 2 * tid;
    bool mine = n < N;
    _Float16* ob = out + row0 * out_stride + (mine ? n : N - 2);
    auto request_out = [&](u32 (&o)[LR_TILE], int blk) {
#pragma unroll
        for (int t = 0; t < LR_TILE; ++t) {
            const int rw = blk * LR_TILE + t < rows ? blk * LR_TILE + t : rows - 1;
            o[t] = *reinterpret_cast<const u32*>(ob + rw * out_stride);
        }
    };
    h8 b0[RK / 8], b1[RK / 8];
    auto request_b = [&]() {
        const _Float16* bp = B + ((size_t)a * N + (mine ? n : N - 2)) * RK;
#pragma unroll
        for (int i = 0; i < RK / 8; ++i) {
            b0[i] = *reinterpret_cast<const h8*>(bp + 8 * i);
            b1[i] = *reinterpret_cast<const h8*>(bp + RK + 8 * i);
        }
    };
    // what does not depend on the planes is requested first, so that its latency runs beside the staging
    u32 o_next[LR_TILE];
    request_out(o_next, 0);
    request_b();

    // ---- 1. t[row, j] = x_scale[row] * (the K-slice planes summed in slice order), all segments, the tile's rows
    lora_stage(s_t, R, tl, R, T, kslices, ws, x_scale);
    __syncthreads();

    // ---- 2. two columns per thread, the tile's 16-row blocks, one column slice after the other (no barrier from here on)
    const float sc = scaling[a];
    const int blocks = (rows + LR_TILE - 1) / LR_TILE;
    for (;;) {
        const int seg = (n >= e0 ? 1 : 0) + (n >= e1 ? 1 : 0);
        for (int blk = 0; blk < blocks; ++blk) {
            u32 o[LR_TILE];
#pragma unroll
            for (int t = 0; t < LR_TILE; ++t) o[t] = o_next[t];
            if (blk + 1 < blocks) request_out(o_next, blk + 1);   // the next block's rows, requested before this block's arithmetic
            // four rows at a time, 8 rank columns at a time: the step's t values (LDS, wave-wide broadcasts) are requested one step
            // ahead, and no instruction moves across a step's end - left alone, the scheduler hoists every LDS read of the block
            // and spills.  All 16 rows: those of a short block past the tile's end are never stored.
            const float* sp = s_t + blk * LR_TILE * R + seg * RK;
            constexpr int PER = RK / 8, STEPS = 4 * PER;
            v4f tb[2][4][2];                             // the t values of this step and the next (static after unrolling)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                tb[0][k][0] = *reinterpret_cast<const v4f*>(sp + k * R);
                tb[0][k][1] = *reinterpret_cast<const v4f*>(sp + k * R + 4);
            }
            float acc0[4], acc1[4];
#pragma unroll
            for (int st = 0; st < STEPS; ++st) {
                const int tq = st / PER, i = st % PER, cb = st & 1;
                if (st + 1 < STEPS) {
                    const float* p = sp + 4 * ((st + 1) / PER) * R + 8 * ((st + 1) % PER);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        tb[cb ^ 1][k][0] = *reinterpret_cast<const v4f*>(p + k * R);
                        tb[cb ^ 1][k][1] = *reinterpret_cast<const v4f*>(p + k * R + 4);
                    }
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (i == 0) acc0[k] = acc1[k] = 0.f;
#pragma unroll
                    for (int h = 0; h < 2; ++h)
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            acc0[k] = __builtin_fmaf((float)b0[i][4 * h + e], tb[cb][k][h][e], acc0[k]);
                            acc1[k] = __builtin_fmaf((float)b1[i][4 * h + e], tb[cb][k][h][e], acc1[k]);
                        }
                }
                if (i == PER - 1) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int t = 4 * tq + k;
                        const u32 y = lora_land(o[t], sc, acc0[k], acc1[k]);
                        if (mine && blk * LR_TILE + t < rows) *reinterpret_cast<u32*>(ob + (blk * LR_TILE + t) * out_stride) = y;
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        ns += gridDim.y;
        if (ns >= nslices) break;                        // (workgroup-uniform)
        n = ns * LR_NSLICE + 2 * tid;
        mine = n < N;
        ob = out + row0 * out_stride + (mine ? n : N - 2);
        request_out(o_next, 0);
        request_b();
    }
}

template <int NJT>
void launch_shrink(dim3 grid, hipStream_t stream, const int8_t* x, long long x_stride, const _Float16* A, const int* seq_adapter, int slots,
                   int K, int R, int rps, int tps, int T, int run, float* ws) {
    hipLaunchKernelGGL(lora_prompt_shrink_kernel<NJT>, grid, dim3(LR_THREADS), 0, stream, x, x_stride, A, seq_adapter, slots, K, R, rps, tps, T,
                       run, ws);
}

template <int RK>
void launch_expand(dim3 grid, size_t lds, hipStream_t stream, _Float16* out, long long out_stride, const _Float16* x_scale, const _Float16* B,
                   const float* scaling, const int* seq_adapter, int slots, int N, int R, int rps, int tps, int T, int kslices, int e0, int e1,
                   const float* ws) {
    hipLaunchKernelGGL(lora_prompt_expand_kernel<RK>, grid, dim3(LR_THREADS), lds, stream, out, out_stride, x_scale, B, scaling, seq_adapter,
                       slots, N, R, rps, tps, T, kslices, e0, e1, ws);
}

}  // namespace

// (the planner's entry points of this form, qs_lora_rows_prompt_run and qs_lora_rows_form_for_rank, stand with the others in lora_rows.hip)
extern "C" int qs_lora_rows_prompt(void* out, int64_t out_stride, const int8_t* x, int64_t x_stride, const void* x_scale, const void* A,
                                   const void* B, const float* scaling, const int32_t* seq_adapter, int slots, int T, int K, int N, int r,
                                   int rows_per_seq, int nseg, int seg_end0, int seg_end1, int seg_end2, void* workspace,
                                   int64_t workspace_size, qs_stream_t stream) {
    LoraCall c;
    int rc = lora_prologue("lora_rows_prompt", c, out, out_stride, x, x_stride, x_scale, A, B, scaling, seq_adapter, slots, T, K, N, r,
                           rows_per_seq, nseg, seg_end0, seg_end1, seg_end2, workspace, workspace_size);
    if (rc != QS_OK) return rc;
    const char* why = lora_plan::prompt_refusal(T, rows_per_seq, slots);
    QS_REQUIRE(!why, "lora_rows_prompt: T=%d, rows_per_seq=%d, slots=%d: %s", T, rows_per_seq, slots, why);
    if (T == 0) return QS_OK;
    const int R = c.R, tps = (rows_per_seq + LP_TILE - 1) / LP_TILE, tiles = lora_plan::prompt_tiles(T, rows_per_seq);
    const int run = lora_plan::prompt_run(tiles, c.kslices);
    // rank groups: the R / 16 (rounded up) rank tiles split evenly over as few groups of at most four (LR_JGROUP rows) as hold them
    const int jtiles = (R + 15) / 16, jgroups = (jtiles + 3) / 4, njt = (jtiles + jgroups - 1) / jgroups;
    const dim3 sgrid(tiles, (c.kslices + run - 1) / run, jgroups);
    const hipStream_t st = (hipStream_t)stream;
#define QS_SHRINK(NJT)                                                                                                                    \
    launch_shrink<NJT>(sgrid, st, x, (long long)x_stride, c.A, seq_adapter, slots, K, R, rows_per_seq, tps, T, run, c.ws)
    switch (njt) {
        case 1: QS_SHRINK(1); break;
        case 2: QS_SHRINK(2); break;
        case 3: QS_SHRINK(3); break;
        default: QS_SHRINK(4); break;
    }
#undef QS_SHRINK
    rc = qs_launch_status("lora_rows_prompt (shrink)");
    if (rc != QS_OK) return rc;
    const dim3 egrid(tiles, lora_plan::prompt_expand_ysplit(tiles, c.nslices));
    const size_t lds = (size_t)LP_TILE * R * sizeof(float);
#define QS_EXPAND(RK)                                                                                                                       \
    launch_expand<RK>(egrid, lds, st, c.out, (long long)out_stride, c.x_scale, c.B, scaling, seq_adapter, slots, N, R, rows_per_seq, tps, T, \
                      c.kslices, c.e0, c.e1, c.ws)
    switch (r) {
        case 8: QS_EXPAND(8); break;
        case 16: QS_EXPAND(16); break;
        case 32: QS_EXPAND(32); break;
        default: QS_EXPAND(64); break;
    }
#undef QS_EXPAND
    return qs_launch_status("lora_rows_prompt (expand)");
}
