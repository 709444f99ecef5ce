// score_rows.hip -- score given tokens under the fp16 lm_head without a logit matrix, for MI355X (gfx950): per row r of `hidden` the
// log-probability of targets[r] under softmax(hidden[r] . lm_head^T), the greedy token and the log-sum-exp.  Contract:
// include/qserve_amd.h (qs_score_rows); design and accounting: DESIGN.md "Scoring prompts"; geometry: score_plan.h.
//
// A flash-style walk over the VOCABULARY instead of over keys.  Two launches:
//   score_walk_kernel   workgroup = 8 wave64 = (128 rows, one split of the vocabulary).  It walks its split's vocabulary tiles of 256
//                       columns; per tile it runs K in stages of 64 through a 3-deep LDS ring and folds the finished fp32 logit tile
//                       into per-row running values in registers.  The tile never leaves the accumulators.
//     * products are SWAPPED, logits^T = lm_head hidden^T on v_mfma_f32_32x32x16_f16 (A = 32 lm_head rows, B = 32 hidden rows): a lane
//       then holds 16 logits of ITS OWN row (row = lane & 31; the two lane halves share it), so the maximum, the sum, the arg-max and the
//       target pick-up are per-lane register work with no cross-lane step per tile (flash_tile.h's S^T = K Q^T, for the same reason).
//       Wave (wv, wr) owns columns 64 wv .. + 63 x rows 64 wr .. + 63 of the tile: 2 x 2 MFMA blocks, 64 accumulator registers.
//     * both operands reach LDS by LDS-DMA (gemm_w4a8_moe_tiled.hip's pattern), a stage = 128 hidden rows x 128 B + 256 lm_head rows x
//       128 B = 48 KiB, as 1 KiB pieces of 8 rows: 2 + 4 DMA instructions per wave and stage, every one fetching whole 128-byte lines.
//       The DMA writes lane-linear, so the image's swizzle - 16-byte chunk c of row j sits at position c ^ ((j >> 1) & 7): the 16 lanes
//       of a quarter wave, 16 consecutive rows at one chunk, then cover the 16 positions of a 256-byte bank period once - is applied to
//       the per-lane SOURCE address.
//     * the walk is ONE flat sequence of steps (tile, k stage): step s + 2 is requested before step s is computed, across tile ends, so
//       the fold of a tile runs under the next tile's first stages.  One raw barrier per step; a counted s_waitcnt vmcnt leaves the next
//       step's six DMA instructions in flight across it.
//     * edges are masked, not padded: rows >= rows and lm_head rows >= V are fetched from the last real row (finite data) and masked to
//       -inf in the fold (columns) or never stored (rows).
//     * per lane and row block the running values are {max m, sum s of exp(x - m), best value / lowest index, target logit}.  A tile's 32
//       exponentials are summed on their own and added to s once, so s sees one rounding per tile, not per column.
//     * at the end the two lane halves of a row merge by one exchange, the four column waves through LDS (the ring is dead), and 128
//       threads write the row's record {m, s, target logit, index} for this split.  Every merge has a fixed order: no atomics.
//   score_merge_kernel  one thread per row merges the row's records in ascending split order and writes lp / greedy / lse.
// Bit-identical run to run and under graph replay: every value is a function of the inputs and the plan alone.
#include "common.h"
#include "score_plan.h"

namespace {

using namespace score_plan;
typedef float v16f __attribute__((ext_vector_type(16)));
typedef __attribute__((address_space(3))) void* lptr_t;

constexpr int NWAVES = 8;
constexpr int THREADS = 64 * NWAVES;
constexpr int A_STAGE = TILE_ROWS * STAGE_K * 2;       // hidden image of a stage: 16 KiB
constexpr int B_STAGE = TILE_VOCAB * STAGE_K * 2;      // lm_head image of a stage: 32 KiB
constexpr int STAGE_BYTES = A_STAGE + B_STAGE;
constexpr int LDS_BYTES = DEPTH * STAGE_BYTES;
constexpr int NA = A_STAGE / 1024 / NWAVES;            // DMA instructions per wave and stage: hidden
constexpr int NB = B_STAGE / 1024 / NWAVES;            //                                      lm_head
constexpr int NDMA = NA + NB;
constexpr float LOG2E = 1.4426950408889634f;
static_assert(TILE_ROWS == 128 && TILE_VOCAB == 256 && STAGE_K == 64 && DEPTH == 3, "the wave layout and the ring are written for this tile");
static_assert(4 * TILE_ROWS * 5 * 4 <= LDS_BYTES, "the end-of-walk exchange lives inside the dead ring");

struct ScoreArgs {
    const _Float16* hidden;
    const _Float16* lm_head;
    const int* targets;
    float4* records;
    long long h_stride, w_stride;      // elements
    int rows, V;
    ScorePlan plan;
};

template <int N>
__device__ __forceinline__ void wait_vm() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
__device__ __forceinline__ void raw_barrier() {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}
// (inline asm, not the builtin: gemm_w4a8_moe_tiled.hip says why)
__device__ __forceinline__ void dma16(u32 voff, const void* sbase, u32 lds_addr) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(sbase), "s"(lds_addr) : "memory");
}

// (m, s) of a softmax over a set: m its maximum (-inf for the empty set), s = sum exp(x - m).  The union of two sets, a then b.
__device__ __forceinline__ void merge_sum(float& m, float& s, float mb, float sb) {
    const float mn = fmaxf(m, mb);
    const float mu = mn == -INFINITY ? 0.f : mn;
    s = s * __builtin_amdgcn_exp2f((m - mu) * LOG2E) + sb * __builtin_amdgcn_exp2f((mb - mu) * LOG2E);
    m = mn;
}
// the larger value; among equals the lower index
__device__ __forceinline__ void merge_best(float& v, int& i, float vb, int ib) {
    const bool take = vb > v || (vb == v && ib < i);
    v = take ? vb : v;
    i = take ? ib : i;
}

__global__ __launch_bounds__(THREADS, 1) void score_walk_kernel(const ScoreArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    int rt, sp;
    if (!grid_position(a.plan, (int)blockIdx.x, &rt, &sp)) return;      // surplus workgroup (uniform, before any barrier)

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wv = wave >> 1, wr = wave & 1;
    const int li = lane & 31, hi = lane >> 5;
    const int row0 = rt * TILE_ROWS;
    const int tile0 = sp * a.plan.tiles_per_split;
    const int tile1 = tile0 + a.plan.tiles_per_split < a.plan.vocab_tiles ? tile0 + a.plan.tiles_per_split : a.plan.vocab_tiles;
    const int nk = a.plan.stages;
    const int steps = (tile1 - tile0) * nk;                             // >= 1: no split is empty, K >= 64
    const int V = a.V;
    const u32 lds0 = (u32)(size_t)(lptr_t)smem;

    // ---- DMA sources.  Piece p = 8 rows; lane l of a piece supplies position l & 7 of row 8 p + (l >> 3), i.e. chunk (l & 7) ^ swz(row).
    // Per-lane 32-bit offsets from the TILE's first row (rows beyond the end clamped to the last real one); tile and stage go into the
    // scalar base.  hidden's offsets are the same for every step; lm_head's depend on the tile only through the clamp.
    const int prow = lane >> 3, ppos = lane & 7;
    u32 a_off[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const int j = 8 * (wave + NWAVES * i) + prow;
        const int jc = row0 + j < a.rows ? j : a.rows - 1 - row0;
        a_off[i] = (u32)jc * (u32)a.h_stride * 2u + (u32)((ppos ^ ((j >> 1) & 7)) * 16);
    }
    const uint8_t* const a_base = reinterpret_cast<const uint8_t*>(a.hidden + (size_t)row0 * (size_t)a.h_stride);
    int it = tile0, ik = 0, islot = 0;                                  // the step the next issue() requests
    auto issue = [&]() {
        const u32 dst = lds0 + islot * STAGE_BYTES;
#pragma unroll
        for (int i = 0; i < NA; ++i) dma16(a_off[i], a_base + (size_t)ik * 128, dst + (wave + NWAVES * i) * 1024);
        const int v0 = it * TILE_VOCAB;
        const uint8_t* const b_base = reinterpret_cast<const uint8_t*>(a.lm_head + (size_t)v0 * (size_t)a.w_stride) + (size_t)ik * 128;
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int j = 8 * (wave + NWAVES * i) + prow;
            const int jc = v0 + j < V ? j : V - 1 - v0;
            dma16((u32)jc * (u32)a.w_stride * 2u + (u32)((ppos ^ ((j >> 1) & 7)) * 16), b_base, dst + A_STAGE + (wave + NWAVES * i) * 1024);
        }
        islot = islot + 1 == DEPTH ? 0 : islot + 1;
        if (++ik == nk) ik = 0, ++it;
    };

    // ---- this lane's rows (one per row block) and their targets
    int tgt[2];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
        const int row = row0 + 64 * wr + 32 * rb + li;
        tgt[rb] = row < a.rows ? a.targets[row] : -1;
    }

    issue();
    if (steps > 1) issue();

    // ---- operand readers: row j = 64 w + 32 b + li of an image, chunk 2 kk + hi at position ^ ((j >> 1) & 7) = ^ ((li >> 1) & 7)
    const int swz = (li >> 1) & 7;
    int c_off[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) c_off[kk] = ((2 * kk + hi) ^ swz) * 16;
    const int a_rd = (64 * wr + li) * 128, b_rd = A_STAGE + (64 * wv + li) * 128;      // + 32 rows = 4096 bytes for block 1

    v16f acc[2][2];                                                      // [column block][row block]
#pragma unroll
    for (int vb = 0; vb < 2; ++vb)
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[vb][rb][r] = 0.f;
    float m_run[2] = {-INFINITY, -INFINITY}, s_run[2] = {0.f, 0.f}, best_v[2] = {-INFINITY, -INFINITY}, x_t[2] = {-INFINITY, -INFINITY};
    int best_i[2] = {0x7fffffff, 0x7fffffff};

    int ct = tile0, ck = 0, slot = 0;                                   // the step being computed
    for (int s = 0; s < steps; ++s) {
        // step s has landed: this wave's pieces by the counted wait, every wave's by the barrier - which also says that every wave is
        // done reading step s - 1, whose slot the request below refills
        if (s + 1 < steps) wait_vm<NDMA>();
        else wait_vm<0>();
        raw_barrier();
        if (s + 2 < steps) issue();
        const uint8_t* const st = smem + slot * STAGE_BYTES;
        // the operands of k block kk + 1 are read before the four MFMAs of block kk (two register sets, the order pinned): the matrix
        // pipe does not sit behind an LDS round trip per block
        h8 w[2][2], h[2][2];
        auto read_ops = [&](int kk) {
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                w[kk & 1][b] = *reinterpret_cast<const h8*>(st + b_rd + b * 4096 + c_off[kk]);
                h[kk & 1][b] = *reinterpret_cast<const h8*>(st + a_rd + b * 4096 + c_off[kk]);
            }
        };
        read_ops(0);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            if (kk + 1 < 4) read_ops(kk + 1);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int vb = 0; vb < 2; ++vb)
#pragma unroll
                for (int rb = 0; rb < 2; ++rb)
                    acc[vb][rb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w[kk & 1][vb], h[kk & 1][rb], acc[vb][rb], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        slot = slot + 1 == DEPTH ? 0 : slot + 1;
        if (++ck < nk) continue;

        // ---- a logit tile is complete: acc[vb][rb][r] = x(this lane's row of block rb, column cbase + 32 vb + 8 (r >> 2) + (r & 3))
        const int cbase = ct * TILE_VOCAB + 64 * wv + 4 * hi;
        const bool edge = ct * TILE_VOCAB + TILE_VOCAB > V;             // wave-uniform: the vocabulary's last tile, partly empty
        const int live = V - cbase;                                     // local columns < live exist
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) {
            const int tl = tgt[rb] - cbase;                             // the target as a local column (anything else: not here)
            float tmax = -INFINITY;
#pragma unroll
            for (int vb = 0; vb < 2; ++vb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int c = 32 * vb + 8 * (r >> 2) + (r & 3);
                    float x = acc[vb][rb][r];
                    if (edge) x = c < live ? x : -INFINITY;
                    acc[vb][rb][r] = x;
                    tmax = fmaxf(tmax, x);
                    if (x > best_v[rb]) best_v[rb] = x, best_i[rb] = cbase + c;     // ascending columns: the lowest index of a maximum stays
                    if (tl == c) x_t[rb] = x;
                }
            const float mn = fmaxf(m_run[rb], tmax);
            const float mu = mn == -INFINITY ? 0.f : mn;               // nothing seen yet: keep the exponents finite
            float tsum = 0.f;
#pragma unroll
            for (int vb = 0; vb < 2; ++vb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    tsum += __builtin_amdgcn_exp2f((acc[vb][rb][r] - mu) * LOG2E);
                    acc[vb][rb][r] = 0.f;
                }
            s_run[rb] = s_run[rb] * __builtin_amdgcn_exp2f((m_run[rb] - mu) * LOG2E) + tsum;
            m_run[rb] = mn;
        }
        ck = 0, ++ct;
    }

    // ---- end of the walk: lane halves, then the four column waves, then one record per row
    raw_barrier();                                                      // the ring is dead
    float* const ex = reinterpret_cast<float*>(smem);                   // [wv 4][row 128][5]
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
        const float mo = __shfl_xor(m_run[rb], 32, 64), so = __shfl_xor(s_run[rb], 32, 64), vo = __shfl_xor(best_v[rb], 32, 64);
        const float xo = __shfl_xor(x_t[rb], 32, 64);
        const int io = __shfl_xor(best_i[rb], 32, 64);
        if (hi == 0) {                                                  // own half first, then the upper one
            merge_sum(m_run[rb], s_run[rb], mo, so);
            merge_best(best_v[rb], best_i[rb], vo, io);
            float* const e = ex + ((wv * TILE_ROWS) + 64 * wr + 32 * rb + li) * 5;
            e[0] = m_run[rb], e[1] = s_run[rb], e[2] = fmaxf(x_t[rb], xo), e[3] = best_v[rb], e[4] = __builtin_bit_cast(float, best_i[rb]);
        }
    }
    __syncthreads();
    if (tid < TILE_ROWS) {
        const float* e = ex + tid * 5;
        float m = e[0], sm = e[1], xt = e[2], bv = e[3];
        int bi = __builtin_bit_cast(int, e[4]);
#pragma unroll
        for (int w = 1; w < 4; ++w) {
            e += TILE_ROWS * 5;
            merge_sum(m, sm, e[0], e[1]);
            xt = fmaxf(xt, e[2]);
            merge_best(bv, bi, e[3], __builtin_bit_cast(int, e[4]));
        }
        // the record keeps the best VALUE in its maximum (they are the same number) and the index beside it
        a.records[((size_t)sp * a.plan.row_tiles + rt) * TILE_ROWS + tid] = make_float4(m, sm, xt, __builtin_bit_cast(float, bi));
    }
}

__global__ __launch_bounds__(256) void score_merge_kernel(const float4* __restrict__ records, const int* __restrict__ targets, float* __restrict__ out_lp,
                                                          int* __restrict__ out_greedy, float* __restrict__ out_lse, int rows, int V, const ScorePlan plan) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= rows) return;
    const size_t per_split = (size_t)plan.row_tiles * TILE_ROWS;
    const int t = targets[row];
    const bool scored = t >= 0 && t < V;
    const int t_split = scored ? (t / TILE_VOCAB) / plan.tiles_per_split : -1;       // no address is formed from a target out of range
    float m = -INFINITY, sm = 0.f, bv = -INFINITY, xt = 0.f;
    int bi = 0x7fffffff;
    for (int sp = 0; sp < plan.splits; ++sp) {                          // ascending: a fixed order of roundings
        const float4 r = records[sp * per_split + row];
        merge_sum(m, sm, r.x, r.y);
        merge_best(bv, bi, r.x, __builtin_bit_cast(int, r.w));
        if (sp == t_split) xt = r.z;
    }
    const float ls = logf(sm);
    out_lp[row] = scored ? (xt - m) - ls : __builtin_nanf("");
    if (out_greedy) out_greedy[row] = bi;
    if (out_lse) out_lse[row] = m + ls;
}

}  // namespace

extern "C" int qs_score_rows_plan(int rows, int n_vocab, int K, int splits, long long* plan8) {
    QS_REQUIRE(plan8, "score_rows_plan: null pointer");
    QS_REQUIRE(rows >= 0 && n_vocab >= 8 && n_vocab <= (1 << 22) && K >= STAGE_K && K % STAGE_K == 0 && splits >= 0,
               "score_rows_plan: rows=%d (>= 0), n_vocab=%d (8 .. 4194304), K=%d (a multiple of 64), splits=%d (>= 0)", rows, n_vocab, K, splits);
    const ScorePlan p = plan_score(rows, n_vocab, K, splits);
    const long long v[8] = {TILE_ROWS, TILE_VOCAB, DEPTH, p.row_tiles, p.vocab_tiles, p.splits, p.tiles_per_split, p.workspace_bytes};
    for (int i = 0; i < 8; ++i) plan8[i] = v[i];
    return QS_OK;
}

extern "C" int qs_score_rows_grid_position(int rows, int n_vocab, int K, int splits, int id, int* row_tile, int* split) {
    QS_REQUIRE(row_tile && split, "score_rows_grid_position: null pointer");
    const ScorePlan p = plan_score(rows, n_vocab, K, splits);
    QS_REQUIRE(p.grid > 0 && id >= 0 && id < p.grid, "score_rows_grid_position: id=%d outside the launch of %d workgroups", id, p.grid);
    *row_tile = *split = -1;
    return grid_position(p, id, row_tile, split) ? 1 : 0;
}

extern "C" int64_t qs_score_rows_workspace_bytes(int rows, int n_vocab, int K, int splits) {
    return rows > 0 && n_vocab > 0 && K > 0 ? (int64_t)plan_score(rows, n_vocab, K, splits < 0 ? 0 : splits).workspace_bytes : 0;
}

extern "C" int qs_score_rows_split(const void* hidden, int64_t hidden_stride, const void* lm_head, int64_t lm_head_stride, const int32_t* targets,
                                   int rows, int n_vocab, int K, int splits, float* out_lp, int32_t* out_greedy, float* out_lse, void* workspace,
                                   int64_t workspace_bytes, qs_stream_t stream) {
    QS_REQUIRE(hidden && lm_head && targets && out_lp && workspace, "score_rows: null pointer");
    QS_REQUIRE(K >= STAGE_K && K % STAGE_K == 0, "score_rows: K=%d must be a multiple of 64", K);
    QS_REQUIRE(n_vocab >= 8 && n_vocab <= (1 << 22), "score_rows: n_vocab=%d (8 .. 4194304)", n_vocab);
    QS_REQUIRE(rows >= 0 && rows <= (1 << 24), "score_rows: rows=%d (0 .. 16777216)", rows);
    QS_REQUIRE(splits >= 0, "score_rows: splits=%d (0: the planner's)", splits);
    // (a row stride is at most 2^22 elements: per-lane offsets inside a tile of 256 rows stay 32-bit)
    QS_REQUIRE(hidden_stride >= K && lm_head_stride >= K && hidden_stride % 8 == 0 && lm_head_stride % 8 == 0 && hidden_stride <= (1 << 22) &&
                   lm_head_stride <= (1 << 22),
               "score_rows: row strides %lld / %lld (elements) must hold a row of K=%d, be multiples of 8 and at most 4194304",
               (long long)hidden_stride, (long long)lm_head_stride, K);
    QS_REQUIRE((((uintptr_t)hidden | (uintptr_t)lm_head | (uintptr_t)workspace) & 15) == 0, "score_rows: hidden, lm_head and workspace must be 16-byte aligned");
    QS_REQUIRE((((uintptr_t)targets | (uintptr_t)out_lp | (uintptr_t)out_greedy | (uintptr_t)out_lse) & 3) == 0,
               "score_rows: an int32 / float array is not 4-byte aligned");
    if (rows == 0) return QS_OK;
    const ScorePlan p = plan_score(rows, n_vocab, K, splits);
    QS_REQUIRE(workspace_bytes >= p.workspace_bytes, "score_rows: workspace of %lld bytes, %lld needed (qs_score_rows_workspace_bytes)",
               (long long)workspace_bytes, p.workspace_bytes);
    static bool lds_reserved[QS_MAX_DEVICES] = {};
    if (const hipError_t e = qs_reserve_lds({reinterpret_cast<const void*>(score_walk_kernel)}, LDS_BYTES, lds_reserved); e != hipSuccess) {
        qs_set_error("score_rows: cannot reserve %d bytes of LDS: %s", LDS_BYTES, hipGetErrorString(e));
        return (int)e;
    }
    const ScoreArgs a = {reinterpret_cast<const _Float16*>(hidden), reinterpret_cast<const _Float16*>(lm_head), targets,
                         reinterpret_cast<float4*>(workspace), (long long)hidden_stride, (long long)lm_head_stride, rows, n_vocab, p};
    hipLaunchKernelGGL(score_walk_kernel, dim3((unsigned)p.grid), dim3(THREADS), LDS_BYTES, (hipStream_t)stream, a);
    if (const int rc = qs_launch_status("score_rows (walk)"); rc != QS_OK) return rc;
    hipLaunchKernelGGL(score_merge_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const float4*>(workspace), targets, out_lp, out_greedy, out_lse, rows, n_vocab, p);
    return qs_launch_status("score_rows (merge)");
}

extern "C" int qs_score_rows(const void* hidden, int64_t hidden_stride, const void* lm_head, int64_t lm_head_stride, const int32_t* targets, int rows,
                             int n_vocab, int K, float* out_lp, int32_t* out_greedy, float* out_lse, void* workspace, int64_t workspace_bytes,
                             qs_stream_t stream) {
    return qs_score_rows_split(hidden, hidden_stride, lm_head, lm_head_stride, targets, rows, n_vocab, K, 0, out_lp, out_greedy, out_lse, workspace,
                               workspace_bytes, stream);
}
