// beam_select.hip -- beam search on the device, for MI355X (gfx950): the W best continuations of every group of W rows, handed out to
// slots so that a row with a surviving child keeps its best child in place, and the in-place move of the rows that got another parent.
// DESIGN.md 10 ("Beam search"); the contracts are in include/qserve_amd.h (qs_beam_select, qs_rows_move).  (Its own translation unit:
// the kernel sets of logprob_rows.hip, sample_rows.hip and stop_update.hip are checked contracts; the 16-bit key, the fixed-point
// weight and the passes of the top list below restate logprob_rows.hip's, which stays untouched - the candidate lists are bit-identical
// to what qs_logprob_rows writes for top = W, T = 1.)  This file holds THREE kernels:
//
//   beam_candidates_kernel  one workgroup of 1024 threads per row.  A dead (cum == -inf) or frozen (finished != 0) row writes ids -1 /
//              lp -inf and returns.  A live row walks its logits (256 KB at n = 128 256, L2-resident across the passes) with 16-byte
//              loads, exactly as logprob_rows_kernel does for a top list: the maximum; the exact 64-bit integer sum of the fixed-point
//              weights with the coarse histogram of the listable keys; the threshold value from a workgroup scan and a fine histogram;
//              the selection in index order through workgroup scans (no atomic append); wave 0 orders the at most 32 entries.
//   beam_merge_kernel       one wave per group.  Lane l holds the candidates e = l + 64 i (row e / W, place e % W) as 64-bit integer
//              keys - the order-preserving bits of the fp32 score above the inverted candidate number, 0 for none - in registers.  W
//              rounds of a wave maximum choose the candidates in order (score descending, row ascending, place ascending); ballots
//              give every row its first chosen candidate and every other chosen candidate the next row without one.  Integer
//              operations and ONE fp32 add per score; no atomics, no LDS, no scratch.
//   rows_move_kernel        one workgroup per (tensor, row): row d of every tensor becomes row parent[d] where that differs from d,
//              with 16-byte vectors where the base and the row size allow, bytes otherwise.  A parent outside the batch, or one that
//              is itself a destination, sets error[0] and the row is skipped: every source stays, so nothing is staged.
#include "common.h"

namespace {

typedef unsigned long long u64;
constexpr int TPB = 1024, WAVES = TPB / 64, COARSE = 1024, FINE = 64, MAX_WIDTH = 32, MAX_MOVE = 16, MOVE_TPB = 256;
constexpr int PER_LANE = MAX_WIDTH * MAX_WIDTH / 64;      // candidates a lane of the merge holds at most
constexpr float FIX = 1099511627776.0f;                   // 2^40
constexpr u32 KEY_NEG_INF = 0x03FFu;                      // order_key(0xFC00): a listable logit has a larger key
constexpr float SCALE_T1 = (float)(1.4426950408889634 / 1.0);   // log2(e) / T at T = 1, as logprob_rows.hip forms it

// fp16 bits -> a 16-bit key that orders like the value (-0 is the value +0)
__device__ __forceinline__ u32 order_key(u32 b) {
    if (b == 0x8000u) b = 0;
    return b ^ ((b & 0x8000u) ? 0xFFFFu : 0x8000u);
}

// fp32 bits -> a 32-bit key that orders like the value (-0 is the value +0); -inf -> 0x007FFFFF, every larger value a larger key
__device__ __forceinline__ u32 score_key(float x) {
    u32 b = __builtin_bit_cast(u32, x);
    if (b == 0x80000000u) b = 0;
    return b ^ ((b & 0x80000000u) ? 0xFFFFFFFFu : 0x80000000u);
}

__device__ __forceinline__ u64 fixed_weight(float x, float m, float scale) {
    float w = __builtin_amdgcn_exp2f((x - m) * scale);
    w = w >= 0.f ? (w <= 1.f ? w : 1.f) : 0.f;            // (NaN - a bad row - counts as 0)
    return (u64)(w * FIX);
}

// lp of one logit, every operation an fp32 operation rounded on its own (no fused multiply-add); lgW: log2 of the sum of the weights
__device__ __forceinline__ float log_prob(float x, float m, float scale, float lgW) {
#pragma clang fp contract(off)
    const float a = (x - m) * scale;
    return (a - lgW) * 0.6931471805599453f;
}

__device__ __forceinline__ float add_rounded(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}

__device__ __forceinline__ u64 wave_scan(u64 v, int lane) {   // inclusive
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u64 o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}

__device__ __forceinline__ u64 wave_total(u64 v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}

__device__ __forceinline__ u64 wave_max_u64(u64 v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const u64 o = __shfl_xor(v, s, 64);
        v = o > v ? o : v;
    }
    return v;
}

// inclusive scan over the workgroup in thread order; s_w: WAVES words; total: the sum over the workgroup
__device__ __forceinline__ u64 block_scan(u64 v, u64* s_w, int lane, int wave, u64& total) {
    const u64 inc = wave_scan(v, lane);
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    u64 off = 0, all = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const u64 s = s_w[w];
        off += w < wave ? s : 0;
        all += s;
    }
    __syncthreads();
    total = all;
    return inc + off;
}

__device__ __forceinline__ u32 half_bits(const v4u& bits, int e) { return (bits[e >> 1] >> ((e & 1) * 16)) & 0xFFFFu; }

struct BeamArgs {
    const _Float16* logits;                              // [batch, row_stride]
    long long row_stride;
    int n_vocab;
    const float* cum;                                    // [batch]
    const int* finished;                                 // [batch]
    const long long* tokens;                             // [batch]
    int batch, width;
    int* parent;                                         // [batch]
    long long* next_token;                               // [batch]
    float* cum_out;                                      // [batch]
    int* moved;                                          // [batch] or null
    int* src_rows;                                       // [batch] or null
    int* cand_ids;                                       // [batch, width]
    float* cand_lp;                                      // [batch, width]
};

// grid = batch, 1024 threads.  8 <= n_vocab <= 2^22, 1 <= width <= 32 (the launcher).
__global__ __launch_bounds__(TPB) void beam_candidates_kernel(const BeamArgs a) {
    __shared__ u32 s_ccnt[COARSE];
    __shared__ u32 s_fcnt[FINE];
    __shared__ u64 s_w[WAVES];
    __shared__ u64 s_red[2][WAVES];
    __shared__ u64 s_sel[MAX_WIDTH];                      // key << 32 | ~index: distinct, larger = earlier in the list
    __shared__ float s_v[WAVES];
    __shared__ int s_bin;
    __shared__ u32 s_above, s_thr, s_cab;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = a.n_vocab, top = a.width;
    const size_t o = (size_t)b * (size_t)top;

    // ---- the row's state (workgroup-uniform): only a live row has continuations
    if (a.cum[b] == -INFINITY || a.finished[b] != 0) {
        if (tid < top) {
            a.cand_ids[o + tid] = -1;
            a.cand_lp[o + tid] = -INFINITY;
        }
        return;
    }
    const _Float16* row = a.logits + (size_t)b * (size_t)a.row_stride;
    const float scale = SCALE_T1;
    const int units = (n + 7) >> 3;

    // ---- 1. the maximum
    float bv = -INFINITY;
    for (int un = tid; un < units; un += TPB) {
        const h8 v = *reinterpret_cast<const h8*>(row + (size_t)un * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (un * 8 + e < n) bv = (float)v[e] > bv ? (float)v[e] : bv;
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const float ov = __shfl_xor(bv, s, 64);
        bv = ov > bv ? ov : bv;
    }
    if (lane == 0) s_v[wave] = bv;
    s_ccnt[tid] = 0;                                      // (COARSE == TPB)
    if (tid < FINE) s_fcnt[tid] = 0;
    if (tid == 0) s_bin = -1;
    __syncthreads();
    bv = s_v[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) bv = s_v[w] > bv ? s_v[w] : bv;
    const float mx = bv;

    // ---- 2. W, the coarse histogram of the listable logits (LDS atomics on integer counts: the order of the additions does not show)
    u64 acc = 0;
    u32 fin = 0;
    for (int un = tid; un < units; un += TPB) {
        const h8 v = *reinterpret_cast<const h8*>(row + (size_t)un * 8);
        const v4u bits = __builtin_bit_cast(v4u, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if (un * 8 + e >= n) continue;
            const u32 key = order_key(half_bits(bits, e));
            acc += fixed_weight((float)v[e], mx, scale);
            if (key > KEY_NEG_INF) {
                ++fin;
                atomicAdd(&s_ccnt[key >> 6], 1u);
            }
        }
    }
    acc = wave_total(acc);
    const u64 fins = wave_total((u64)fin);
    if (lane == 0) {
        s_red[0][wave] = acc;
        s_red[1][wave] = fins;
    }
    __syncthreads();
    u64 W = 0, Fn = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        W += s_red[0][w];
        Fn += s_red[1][w];
    }
    float lgW = __builtin_amdgcn_logf((float)W) - 40.f;   // log2 of the sum of the weights
    asm volatile("" : "+v"(lgW));                         // (formed here: the sixteen partial sums do not live until the list is written)
    const int kk = Fn < (u64)top ? (int)Fn : top;         // entries the list holds

    // ---- 3. the threshold: the kk-th largest listable value, and the count of values strictly above it
    if (kk > 0) {
        const int cb = COARSE - 1 - tid;                  // descending: thread 0 owns the bin of the largest values
        const u64 ct = s_ccnt[cb];
        u64 total;
        const u64 cum = block_scan(ct, s_w, lane, wave, total);
        if (cum >= (u64)kk && cum - ct < (u64)kk) {
            s_bin = cb;
            s_above = (u32)(cum - ct);
        }
        __syncthreads();
        const int bin = s_bin;
        for (int un = tid; un < units; un += TPB) {
            const h8 v = *reinterpret_cast<const h8*>(row + (size_t)un * 8);
            const v4u bits = __builtin_bit_cast(v4u, v);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                if (un * 8 + e >= n) continue;
                const u32 key = order_key(half_bits(bits, e));
                if ((int)(key >> 6) == bin && key > KEY_NEG_INF) atomicAdd(&s_fcnt[key & (FINE - 1)], 1u);
            }
        }
        __syncthreads();
        if (wave == 0) {
            const int c = FINE - 1 - lane;                // descending again
            const u64 fc = s_fcnt[c];
            const u64 cumf = (u64)s_above + wave_scan(fc, lane);
            const u64 votes = __ballot(cumf >= (u64)kk);
            const int first = votes ? __ffsll(votes) - 1 : 63;   // (votes != 0: the bin holds the kk-th value)
            if (lane == first) {
                s_thr = ((u32)bin << 6) | (u32)c;
                s_cab = (u32)(cumf - fc);
            }
        }
        __syncthreads();
        const u32 thr = s_thr;
        const int cab = (int)s_cab, need = kk - cab;      // values above the threshold (< kk), ids to take from its class (>= 1)

        // ---- 4. the selection, in index order
        int rg = 0, re = 0;                               // entries placed so far: above the threshold, of its class
        for (int base = 0; base < units && (rg < cab || re < need); base += TPB) {   // (workgroup-uniform)
            const int un = base + tid;
            u32 keys[8];
            u32 g = 0, q = 0;
            if (un < units) {
                const h8 v = *reinterpret_cast<const h8*>(row + (size_t)un * 8);
                const v4u bits = __builtin_bit_cast(v4u, v);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const u32 key = un * 8 + e < n ? order_key(half_bits(bits, e)) : 0u;   // (key 0 is below every threshold)
                    keys[e] = key;
                    g += key > thr;
                    q += key == thr;
                }
            }
            u64 total;
            const u64 inc = block_scan(((u64)g << 32) | (u64)q, s_w, lane, wave, total);
            if (g | q) {
                int pg = rg + (int)(inc >> 32) - (int)g, pq = re + (int)(inc & 0xFFFFFFFFull) - (int)q;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const u64 ent = ((u64)keys[e] << 32) | (u64)(0xFFFFFFFFu - (u32)(un * 8 + e));
                    if (keys[e] > thr) {
                        if (pg < cab) s_sel[pg] = ent;    // (always: cab counts exactly these)
                        ++pg;
                    } else if (keys[e] == thr) {
                        if (pq < need) s_sel[cab + pq] = ent;
                        ++pq;
                    }
                }
            }
            rg += (int)(total >> 32);
            re += (int)(total & 0xFFFFFFFFull);
        }
        __syncthreads();
    }

    // ---- 5. the list: wave 0 orders the entries and writes them
    if (wave != 0 || lane >= top) return;
    int id = -1, pos = lane;
    float lp = -INFINITY;
    if (lane < kk) {
        const u64 mine = s_sel[lane];
        pos = 0;
        for (int i = 0; i < kk; ++i) pos += s_sel[i] > mine;
        id = (int)(0xFFFFFFFFu - (u32)(mine & 0xFFFFFFFFull));
        lp = log_prob((float)row[id], mx, scale, lgW);
    }
    a.cand_ids[o + pos] = id;
    a.cand_lp[o + pos] = lp;
}

// grid = batch / width groups, one wave each.  Every index below is a lane number, a loop counter or derived from them: cand_ids
// only ever become tokens, never addresses.
__global__ __launch_bounds__(64) void beam_merge_kernel(const BeamArgs a) {
    const int g = blockIdx.x, lane = threadIdx.x, W = a.width, r0 = g * W, total = W * W;

    // ---- the candidates of this lane as keys: score bits above the inverted candidate number (row-major: row, then place)
    u64 keys[PER_LANE];
#pragma unroll
    for (int i = 0; i < PER_LANE; ++i) {
        const int e = lane + 64 * i;
        u64 key = 0;
        if (e < total) {
            const int q = e / W, r = e - q * W, b = r0 + q;
            const float c = a.cum[b];
            const bool dead = c == -INFINITY, frozen = !dead && a.finished[b] != 0;
            float score = -INFINITY;
            if (frozen) {
                if (r == 0) score = c;
            } else if (!dead) {
                if (a.cand_ids[(size_t)b * W + r] >= 0) score = add_rounded(c, a.cand_lp[(size_t)b * W + r]);
            }
            if (score > -INFINITY) key = ((u64)score_key(score) << 32) | (u64)(0xFFFFFFFFu - (u32)e);   // (NaN is dropped too)
        }
        keys[i] = key;
    }

    // ---- W rounds: the largest key left is the next chosen candidate; lane c keeps the c-th
    u64 mine = 0;
    for (int c = 0; c < W; ++c) {                         // (wave-uniform)
        u64 best = 0;
#pragma unroll
        for (int i = 0; i < PER_LANE; ++i) best = keys[i] > best ? keys[i] : best;
        best = wave_max_u64(best);
        if (best == 0) break;
#pragma unroll
        for (int i = 0; i < PER_LANE; ++i)
            if (keys[i] == best) keys[i] = 0;             // (keys are distinct: exactly one entry of one lane)
        if (lane == c) mine = best;
    }
    const bool chosen = mine != 0;                        // lanes 0 .. count - 1
    const int e = chosen ? (int)(0xFFFFFFFFu - (u32)(mine & 0xFFFFFFFFull)) : 0;
    const int p = e / W, r = e - p * W;                   // the candidate's row in the group, its place in the row's list

    // ---- slots: a row's first chosen candidate stays in the row; the others take the rows without one, both in ascending order
    bool first = false;
    int src = -1;                                         // the chosen candidate (a lane) that lands in slot `lane`; -1: none
    for (int q = 0; q < W; ++q) {
        const u64 m = __ballot(chosen && p == q);         // the chosen candidates of row q; the lowest lane is its best
        const int best = m ? __ffsll(m) - 1 : -1;
        if (chosen && p == q) first = best == lane;
        if (lane == q) src = best;
    }
    const bool hole = lane < W && src < 0;
    const u64 extras = __ballot(chosen && !first), holes = __ballot(hole);
    const int hole_rank = __popcll(holes & ((1ull << lane) - 1ull));
    int seen = 0;
    for (int c = 0; c < W; ++c) {                         // the k-th further candidate takes the k-th row without one
        if ((extras >> c) & 1ull) {
            if (hole && hole_rank == seen) src = c;
            ++seen;
        }
    }

    // ---- the chosen candidates' rows, tokens and scores, from the lanes that hold them
    const int bp = r0 + p;
    float score = -INFINITY;
    long long token = 0;
    if (chosen) {
        const float c = a.cum[bp];
        if (a.finished[bp] != 0) {
            score = c;
            token = a.tokens[bp];
        } else {
            score = add_rounded(c, a.cand_lp[(size_t)bp * W + r]);
            token = (long long)a.cand_ids[(size_t)bp * W + r];
        }
    }
    const int from = src < 0 ? lane : src;
    const int sp = __shfl(bp, from, 64);
    const float ss = __shfl(score, from, 64);
    const long long st = __shfl(token, from, 64);
    if (lane >= W) return;
    const int d = r0 + lane;
    const int par = src < 0 ? d : sp;
    const long long own_token = a.tokens[d];
    a.parent[d] = par;
    a.next_token[d] = src < 0 ? own_token : st;
    a.cum_out[d] = src < 0 ? -INFINITY : ss;
    if (a.moved) a.moved[d] = par != d;
    if (a.src_rows) a.src_rows[d] = par != d ? par : -1;
}

struct MoveArgs {
    const int* parent;                                   // [batch]
    int* error;                                          // [1]
    int batch, num;
    unsigned char* base[MAX_MOVE];
    long long row_bytes[MAX_MOVE];
};

// grid = (num, batch), 256 threads
__global__ __launch_bounds__(MOVE_TPB) void rows_move_kernel(const MoveArgs a) {
    const int t = blockIdx.x, d = blockIdx.y, tid = threadIdx.x;
    const int p = a.parent[d];
    if (p == d) return;
    if (p < 0 || p >= a.batch || a.parent[p] != p) {      // (the second read only for p inside the batch)
        if (tid == 0 && t == 0) a.error[0] = 1;
        return;
    }
    unsigned char* base = a.base[0];
    long long bytes = a.row_bytes[0];
#pragma unroll
    for (int i = 1; i < MAX_MOVE; ++i)                    // (a select chain: a dynamic index into the argument would go through scratch)
        if (i == t) {
            base = a.base[i];
            bytes = a.row_bytes[i];
        }
    const unsigned char* src = base + (size_t)p * (size_t)bytes;
    unsigned char* dst = base + (size_t)d * (size_t)bytes;
    if ((((uintptr_t)base | (uintptr_t)bytes) & 15) == 0) {
        const long long vecs = bytes >> 4;
        for (long long i = tid; i < vecs; i += MOVE_TPB) reinterpret_cast<v4u*>(dst)[i] = reinterpret_cast<const v4u*>(src)[i];
    } else {
        for (long long i = tid; i < bytes; i += MOVE_TPB) dst[i] = src[i];
    }
}

}  // namespace

extern "C" int qs_beam_select(const void* logits, int64_t row_stride, int n_vocab, const float* cum, const int32_t* finished,
                              const int64_t* tokens, int batch, int width, int32_t* parent, int64_t* next_token, float* cum_out,
                              int32_t* moved, int32_t* src_rows, int32_t* cand_ids, float* cand_lp, qs_stream_t stream) {
    QS_REQUIRE(logits && cum && finished && tokens && parent && next_token && cum_out && cand_ids && cand_lp, "beam_select: null pointer");
    QS_REQUIRE(width >= 1 && width <= MAX_WIDTH, "beam_select: width=%d (1 .. %d)", width, MAX_WIDTH);
    QS_REQUIRE(batch >= 0 && batch <= 65535, "beam_select: batch=%d (0 .. 65535, one workgroup per row)", batch);
    QS_REQUIRE(batch % width == 0, "beam_select: batch=%d is not a multiple of width=%d (rows g * width .. g * width + width - 1 form group g)",
               batch, width);
    QS_REQUIRE(n_vocab >= 8 && n_vocab <= (1 << 22) && row_stride >= n_vocab && row_stride % 8 == 0,
               "beam_select: n_vocab=%d (8 .. 4194304), row stride %lld (must be >= n_vocab, multiple of 8)", n_vocab, (long long)row_stride);
    QS_REQUIRE(cum_out != cum, "beam_select: cum_out must not alias cum (a group reads the scores of all its rows while it writes)");
    QS_REQUIRE(((uintptr_t)logits & 15) == 0, "beam_select: logits must be 16-byte aligned");
    QS_REQUIRE((((uintptr_t)tokens | (uintptr_t)next_token) & 7) == 0, "beam_select: tokens and next_token must be 8-byte aligned");
    const uintptr_t words = (uintptr_t)cum | (uintptr_t)finished | (uintptr_t)parent | (uintptr_t)cum_out | (uintptr_t)moved |
                            (uintptr_t)src_rows | (uintptr_t)cand_ids | (uintptr_t)cand_lp;
    QS_REQUIRE((words & 3) == 0, "beam_select: an int32 / float array is not 4-byte aligned");
    if (batch == 0) return QS_OK;
    BeamArgs a;
    a.logits = (const _Float16*)logits, a.row_stride = (long long)row_stride, a.n_vocab = n_vocab;
    a.cum = cum, a.finished = finished, a.tokens = (const long long*)tokens, a.batch = batch, a.width = width;
    a.parent = parent, a.next_token = (long long*)next_token, a.cum_out = cum_out, a.moved = moved, a.src_rows = src_rows;
    a.cand_ids = cand_ids, a.cand_lp = cand_lp;
    hipLaunchKernelGGL(beam_candidates_kernel, dim3(batch), dim3(TPB), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(beam_merge_kernel, dim3(batch / width), dim3(64), 0, (hipStream_t)stream, a);
    return qs_launch_status("beam_select");
}

extern "C" int qs_rows_move(const int32_t* parent, int batch, const void* const* bases, const int64_t* row_bytes, int num, int32_t* error,
                            qs_stream_t stream) {
    QS_REQUIRE(parent && error, "rows_move: null pointer");
    QS_REQUIRE(batch >= 0 && batch <= 65535, "rows_move: batch=%d (0 .. 65535, one grid row per row)", batch);
    QS_REQUIRE(num >= 0 && num <= MAX_MOVE, "rows_move: num=%d tensors (0 .. %d: they travel in the kernel argument)", num, MAX_MOVE);
    QS_REQUIRE(num == 0 || (bases && row_bytes), "rows_move: null pointer (num=%d needs bases and row_bytes)", num);
    QS_REQUIRE((((uintptr_t)parent | (uintptr_t)error) & 3) == 0, "rows_move: an int32 array is not 4-byte aligned");
    MoveArgs a;
    a.parent = parent, a.error = error, a.batch = batch, a.num = num;
    for (int i = 0; i < MAX_MOVE; ++i) {
        a.base[i] = nullptr;
        a.row_bytes[i] = 0;
    }
    for (int i = 0; i < num; ++i) {
        QS_REQUIRE(bases[i] && row_bytes[i] >= 1 && row_bytes[i] <= (int64_t)1 << 31,
                   "rows_move: tensor %d: base %p, row_bytes=%lld (a base address and 1 .. 2^31 bytes per row)", i, bases[i],
                   (long long)row_bytes[i]);
        a.base[i] = (unsigned char*)bases[i];
        a.row_bytes[i] = (long long)row_bytes[i];
    }
    if (batch == 0 || num == 0) return QS_OK;
    hipLaunchKernelGGL(rows_move_kernel, dim3(num, batch), dim3(MOVE_TPB), 0, (hipStream_t)stream, a);
    return qs_launch_status("rows_move");
}
