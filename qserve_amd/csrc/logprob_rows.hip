// logprob_rows.hip -- log-probabilities of the tokens a round emits, for MI355X (gfx950): per emitted token its log-probability, its rank
// and a short top list, on the device, from the fp16 logit rows of a decode step or of the accepted path of a tree verification.
// DESIGN.md 10 ("Log-probabilities"); the contract is in include/qserve_amd.h (qs_logprob_rows).  (Its own translation unit: the kernel
// sets of sample_rows.hip and stop_update.hip are checked contracts; the 16-bit key and the fixed-point weight below restate
// sample_rows.hip's, which stays untouched.)  This file holds ONE kernel:
//
//   logprob_rows_kernel  one workgroup of 1024 threads per (slot, sequence); a slot that is not live, or whose column is beyond the
//              output, returns at once.  A live slot gathers its row and its id from the walk's outputs (the e_j of qs_stop_update),
//              then walks the row (256 KB at n = 128 256, L2-resident across the passes) with 16-byte loads:
//                1. the maximum m.
//                2. W = sum floor(exp2((x_i - m) * log2(e) / T) * 2^40), an exact 64-bit integer sum (the sampler's weights), and in
//                   the same pass the two integer counts of the rank - keys above the id's key, equal keys in front of the id - and,
//                   with a top list, the count of listable (not -inf) logits per coarse bin (the upper 10 bits of the key; LDS atomics
//                   on integer counts: the order of the additions does not show).
//                3. only with a top list: a descending workgroup scan finds the coarse bin that holds the kk-th largest listable value
//                   (kk = min(top, listable)), a second histogram over that bin's 64 values and a wave scan find the value itself:
//                   the threshold, a VALUE, and how many values lie strictly above it.
//                4. the selection, 1024 units at a time in index order: every thread counts the elements of its unit above and at the
//                   threshold, one workgroup scan of the packed pair gives each element its place - all values above the threshold,
//                   then the FIRST remaining ids of the threshold class in index order.  No atomic append: the places are a function
//                   of the row alone.  The loop ends as soon as the list is full.
//                5. wave 0 sorts the at most 32 entries by (key descending, index ascending) - entries are distinct 48-bit integers,
//                   each lane counts the larger ones - and writes ids and log-probabilities; the tail is id -1, -inf.
//              Elements behind n in the last 16-byte unit are masked by index in every pass.  No scratch, no workspace; 5 KB of LDS.
#include "common.h"

namespace {

typedef unsigned long long u64;
constexpr int TPB = 1024, WAVES = TPB / 64, COARSE = 1024, FINE = 64, MAX_TOP = 32, MAX_NODES = 64;
constexpr float FIX = 1099511627776.0f;                   // 2^40
constexpr u32 KEY_NEG_INF = 0x03FFu;                      // order_key(0xFC00): a listable logit has a larger key

// fp16 bits -> a 16-bit key that orders like the value (-0 is the value +0)
__device__ __forceinline__ u32 order_key(u32 b) {
    if (b == 0x8000u) b = 0;
    return b ^ ((b & 0x8000u) ? 0xFFFFu : 0x8000u);
}

__device__ __forceinline__ u64 fixed_weight(float x, float m, float scale) {
    float w = __builtin_amdgcn_exp2f((x - m) * scale);
    w = w >= 0.f ? (w <= 1.f ? w : 1.f) : 0.f;            // (NaN - a bad row - counts as 0)
    return (u64)(w * FIX);
}

// lp of one logit, every operation an fp32 operation rounded on its own (no fused multiply-add): the chosen id's value and its entry in
// the top list are the same bits.  lgW: log2 of the sum of the weights
__device__ __forceinline__ float log_prob(float x, float m, float scale, float lgW) {
#pragma clang fp contract(off)
    const float a = (x - m) * scale;
    return (a - lgW) * 0.6931471805599453f;
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

__device__ __forceinline__ int clamp_node(int idx, int n) { return idx < 0 ? 0 : idx >= n ? n - 1 : idx; }

struct LogprobArgs {
    const _Float16* logits;                              // [batch * n, row_stride]
    long long row_stride;
    int n_vocab;
    const long long* node_tokens;                        // [batch, n] or null
    const int* accept_idx;                               // [batch, max_accept] or null
    const int* accept_lens;                              // [batch] or null (m = 1)
    const long long* next_token;                         // [batch]
    const int* lengths;                                  // [batch] or null (column j - 1)
    int batch, n, max_accept;
    float temperature;
    const float* seq_temperature;                        // [batch] or null
    int top;
    float* out_lp;                                       // [batch, out_stride]
    int* out_rank;                                       // [batch, out_stride] or null
    int* out_top_ids;                                    // [batch, out_stride, top]
    float* out_top_lp;                                   // [batch, out_stride, top]
    long long out_stride;
    int out_cols;
};

// grid = (max_accept, batch), 1024 threads.  8 <= n_vocab <= 2^22, 1 <= n, max_accept <= 64, 0 <= top <= 32 (the launcher).
__global__ __launch_bounds__(TPB) void logprob_rows_kernel(const LogprobArgs a) {
    __shared__ u32 s_ccnt[COARSE];
    __shared__ u32 s_fcnt[FINE];
    __shared__ u64 s_w[WAVES];
    __shared__ u64 s_red[3][WAVES];
    __shared__ u64 s_sel[MAX_TOP];                        // key << 32 | ~index: distinct, larger = earlier in the list
    __shared__ float s_v[WAVES];
    __shared__ int s_bin;
    __shared__ u32 s_above, s_thr, s_cab;
    const int b = blockIdx.y, j = blockIdx.x + 1, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = a.n_vocab, top = a.top;

    // ---- the slot (workgroup-uniform): live?  its column, its row, its id
    int mcap = a.max_accept < MAX_NODES ? a.max_accept : MAX_NODES;
    if (!a.node_tokens || !a.accept_idx) mcap = 1;        // (a plain batch of rows: the one slot scores next_token)
    int m = a.accept_lens ? a.accept_lens[b] : 1;
    m = m < 0 ? 0 : m > mcap ? mcap : m;
    if (j > m) return;
    long long col = j - 1;
    if (a.lengths) {
        const int L = a.lengths[b];
        col = (long long)(L < 0 ? 0 : L) - 1 + j;
    }
    if (col >= (long long)a.out_cols) return;
    const size_t idx_row = (size_t)b * a.max_accept;
    const int node = a.accept_idx ? clamp_node(a.accept_idx[idx_row + j - 1], a.n) : 0;
    const _Float16* row = a.logits + ((size_t)b * a.n + node) * (size_t)a.row_stride;
    const long long t64 = j < m ? a.node_tokens[(size_t)b * a.n + clamp_node(a.accept_idx[idx_row + j], a.n)] : a.next_token[b];
    const bool t_ok = t64 >= 0 && t64 < (long long)n;
    const int t = t_ok ? (int)t64 : -1;
    const size_t o = (size_t)b * (size_t)a.out_stride + (size_t)col;
    float T = a.seq_temperature ? a.seq_temperature[b] : a.temperature;
    if (!(T >= 1e-5f)) T = 1.f;                           // a greedy row (a NaN parameter too) reports the untempered distribution
    const float scale = (float)(1.4426950408889634 / (double)T);
    const int units = (n + 7) >> 3;
    const _Float16 xt_h = t_ok ? row[t] : (_Float16)0.f;
    const float xt = (float)xt_h;
    const u32 key_t = order_key((u32)__builtin_bit_cast(unsigned short, xt_h));

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

    // ---- 2. W, the rank's counts, the coarse histogram of the listable logits
    u64 acc = 0;
    u32 gt = 0, eqb = 0, fin = 0;
    for (int un = tid; un < units; un += TPB) {
        const h8 v = *reinterpret_cast<const h8*>(row + (size_t)un * 8);
        const v4u bits = __builtin_bit_cast(v4u, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int i = un * 8 + e;
            if (i >= n) continue;
            const u32 key = order_key(half_bits(bits, e));
            acc += fixed_weight((float)v[e], mx, scale);
            gt += key > key_t;
            eqb += key == key_t && i < t;
            if (top > 0 && key > KEY_NEG_INF) {
                ++fin;
                atomicAdd(&s_ccnt[key >> 6], 1u);
            }
        }
    }
    acc = wave_total(acc);
    const u64 cnts = wave_total(((u64)gt << 32) | (u64)eqb);  // (each count <= n <= 2^22: the halves do not meet)
    const u64 fins = wave_total((u64)fin);
    if (lane == 0) {
        s_red[0][wave] = acc;
        s_red[1][wave] = cnts;
        s_red[2][wave] = fins;
    }
    __syncthreads();
    u64 W = 0, C = 0, Fn = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        W += s_red[0][w];
        C += s_red[1][w];
        Fn += s_red[2][w];
    }
    const float lgW = __builtin_amdgcn_logf((float)W) - 40.f;   // log2 of the sum of the weights
    if (tid == 0) {
        a.out_lp[o] = t_ok ? log_prob(xt, mx, scale, lgW) : __builtin_nanf("");
        if (a.out_rank) a.out_rank[o] = t_ok ? 1 + (int)(C >> 32) + (int)(C & 0xFFFFFFFFull) : 0;
    }
    if (top <= 0) return;
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
    a.out_top_ids[o * (size_t)top + pos] = id;
    a.out_top_lp[o * (size_t)top + pos] = lp;
}

}  // namespace

extern "C" int qs_logprob_rows(const void* logits, int64_t row_stride, int n_vocab, const int64_t* node_tokens, const int32_t* accept_idx,
                               const int32_t* accept_lens, const int64_t* next_token, const int32_t* lengths, int batch, int n,
                               int max_accept, float temperature, const float* seq_temperature, int top, float* out_lp, int32_t* out_rank,
                               int32_t* out_top_ids, float* out_top_lp, int64_t out_stride, int out_cols, qs_stream_t stream) {
    QS_REQUIRE(logits && next_token && out_lp, "logprob_rows: null pointer");
    QS_REQUIRE(n_vocab >= 8 && n_vocab <= (1 << 22) && row_stride >= n_vocab && row_stride % 8 == 0,
               "logprob_rows: n_vocab=%d (8 .. 4194304), row stride %lld (must be >= n_vocab, multiple of 8)", n_vocab, (long long)row_stride);
    QS_REQUIRE(n >= 1 && n <= MAX_NODES, "logprob_rows: n=%d, a tree has 1 .. %d nodes", n, MAX_NODES);
    QS_REQUIRE(max_accept >= 1 && max_accept <= MAX_NODES, "logprob_rows: max_accept=%d, a path has 1 .. %d nodes", max_accept, MAX_NODES);
    QS_REQUIRE(top >= 0 && top <= MAX_TOP, "logprob_rows: top=%d (0 .. %d)", top, MAX_TOP);
    QS_REQUIRE(top == 0 || (out_top_ids && out_top_lp), "logprob_rows: null pointer (top=%d needs out_top_ids and out_top_lp)", top);
    QS_REQUIRE(node_tokens || n == 1, "logprob_rows: node_tokens is null with n=%d (only a plain batch of rows, n = 1, has no draft)", n);
    QS_REQUIRE(accept_idx || max_accept == 1, "logprob_rows: accept_idx is null with max_accept=%d", max_accept);
    QS_REQUIRE(out_cols >= 0 && out_stride >= out_cols, "logprob_rows: out_cols=%d, out_stride=%lld (0 <= out_cols <= out_stride)", out_cols,
               (long long)out_stride);
    QS_REQUIRE(batch >= 0 && batch <= 65535, "logprob_rows: batch=%d (0 .. 65535, one grid row per sequence)", batch);
    QS_REQUIRE(((uintptr_t)logits & 15) == 0, "logprob_rows: logits must be 16-byte aligned");
    QS_REQUIRE((((uintptr_t)node_tokens | (uintptr_t)next_token) & 7) == 0, "logprob_rows: node_tokens and next_token must be 8-byte aligned");
    const uintptr_t words = (uintptr_t)accept_idx | (uintptr_t)accept_lens | (uintptr_t)lengths | (uintptr_t)seq_temperature | (uintptr_t)out_lp |
                            (uintptr_t)out_rank | (uintptr_t)out_top_ids | (uintptr_t)out_top_lp;
    QS_REQUIRE((words & 3) == 0, "logprob_rows: an int32 / float array is not 4-byte aligned");
    if (batch == 0) return QS_OK;
    LogprobArgs a;
    a.logits = (const _Float16*)logits, a.row_stride = (long long)row_stride, a.n_vocab = n_vocab;
    a.node_tokens = (const long long*)node_tokens, a.accept_idx = accept_idx, a.accept_lens = accept_lens;
    a.next_token = (const long long*)next_token, a.lengths = lengths;
    a.batch = batch, a.n = n, a.max_accept = max_accept;
    a.temperature = temperature, a.seq_temperature = seq_temperature, a.top = top;
    a.out_lp = out_lp, a.out_rank = out_rank, a.out_top_ids = out_top_ids, a.out_top_lp = out_top_lp;
    a.out_stride = (long long)out_stride, a.out_cols = out_cols;
    hipLaunchKernelGGL(logprob_rows_kernel, dim3(max_accept, batch), dim3(TPB), 0, (hipStream_t)stream, a);
    return qs_launch_status("logprob_rows");
}
