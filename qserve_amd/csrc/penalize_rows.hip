// penalize_rows.hip -- repetition, presence and frequency penalties on fp16 logit rows, for MI355X (gfx950): the step in front of the
// sampling head (qs_argmax_rows / qs_sample_rows) of the decode step and of tree verification, on the device.  DESIGN.md 10
// ("Penalties"); the rule is the header comment of qs_penalize_rows in include/qserve_amd.h.  (Its own translation unit: the kernel sets
// of sample_rows.hip and ngram_draft.hip are checked contracts.)  This file holds ONE kernel:
//
//   penalize_rows_kernel  one workgroup of 1024 threads per (vocabulary slice of 32 768 ids, sequence); no cross-workgroup communication,
//              no waits, no scratch.  A workgroup touches only its own slice of its own sequence's rows, so the in-place edit is race-free.
//                1. neutral sequences (rep == 1, freq == 0, pres == 0) leave at once: nothing of theirs is read or written.
//                2. the history h[0 .. L) is counted ONCE into s_cnt, one 32-bit LDS word per id of the slice - c_all in the low half,
//                   c_gen (positions >= prompt_lens[b]) in the high half - with one LDS atomicAdd per token that falls into the slice
//                   (16-byte loads where the row is 16-byte aligned, coalesced 4-byte loads otherwise).  Integer counts: order-free, so
//                   the result is bit-identical run to run.  Counts stay below 2^16 because the launcher refuses cap + 63 > 65 535.
//                3. thread t owns the words t, t + 1024, ... (conflict-free, and neighbouring lanes edit neighbouring logits) and keeps
//                   the 32-bit mask of its non-zero words in a register: a row's walk reads only those.  Lane l of wave 0 keeps node
//                   l's token, its base count and the mask of the lanes that hold the same token; s_anc[i] is the mask of the nodes
//                   != 0 on the path root -> i (a malformed parent entry: the node alone, and its children hang off it as they do for
//                   the drafter).
//                4. per row i: the path's tokens are marked in s_mark (bit k of word t <=> id t + 1024 k: the layout of the owners'
//                   masks), one barrier, then every owner edits its non-zero, unmarked ids from the LDS counts while in wave 0 the
//                   first lane of every distinct path token edits it with base count + multiplicity on the path - each logit is read
//                   and written once.  Three mark buffers in rotation: the marks of row i are cleared behind the barrier of row i + 1
//                   and set again no earlier than row i + 3, so one barrier per row orders everything.  (Two buffers would put the
//                   clear of a word by one lane and the next atomicOr into it by ANOTHER lane of wave 0 between the same two
//                   barriers, ordered by nothing but the wave's instruction order - which the hardware keeps and the language
//                   does not promise across lanes.  The third buffer, 4 KiB, puts a barrier between them instead of a fence.)
//              The edit rounds every fp32 operation on its own (no contraction into an FMA), so a float32 restatement is bit-equal.
//              Static LDS: s_cnt 128 KiB + s_mark 12 KiB + s_anc 512 B + s_par 256 B.
#include "common.h"

namespace {

constexpr int PEN_THREADS = 1024;
constexpr int PEN_SLICE = 32768;                     // ids per workgroup = words of s_cnt
constexpr int PEN_OWNED = PEN_SLICE / PEN_THREADS;   // words per thread: the bits of its mask
constexpr int PEN_MAX_NODES = 64;
constexpr int PEN_MAX_COUNT = 65535;                 // cap + 63 must not exceed it: 16-bit counts
constexpr int PEN_MAX_BATCH = 65535;                 // sequences per launch: the grid's y extent
static_assert(PEN_OWNED == 32, "an owner's mask is one 32-bit word");

typedef unsigned long long u64;

// one logit under the counts `cnt` (c_all | c_gen << 16, c_all > 0).  -inf stays -inf, untouched.  Every operation is rounded on its
// own: contraction is off for the body (the __fmul_rn family are plain operators in inline functions of their own, compiled under the
// translation unit's default, so the operators stand here), and the division is the correctly rounded one (hipcc's default).
__device__ __forceinline__ void edit(_Float16* p, u32 cnt, float rep, float freq, float pres) {
#pragma clang fp contract(off)
    float x = (float)*p;
    if (x == -INFINITY) return;
    const u32 c_gen = cnt >> 16;
    x = x > 0.f ? x / rep : x * rep;
    float pen = freq * (float)c_gen;
    pen = pen + (c_gen > 0 ? pres : 0.f);
    x = x - pen;
    *p = (_Float16)x;
}

// grid = (slices, sequences), 1024 threads.  The launcher checks n, the strides, n_nodes and cap.
__global__ __launch_bounds__(PEN_THREADS) void penalize_rows_kernel(_Float16* __restrict__ logits, long long row_stride, int n,
                                                                    const int* __restrict__ history, long long hist_stride, int cap,
                                                                    const int* __restrict__ lengths, const int* __restrict__ prompt_lens,
                                                                    const long long* __restrict__ node_tokens,
                                                                    const int* __restrict__ parents, int n_nodes, float rep, float freq,
                                                                    float pres, const float* __restrict__ seq_rep,
                                                                    const float* __restrict__ seq_freq, const float* __restrict__ seq_pres) {
    __shared__ u32 s_cnt[PEN_SLICE];
    __shared__ u32 s_mark[3 * PEN_THREADS];
    __shared__ u64 s_anc[PEN_MAX_NODES];
    __shared__ int s_par[PEN_MAX_NODES];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lo = blockIdx.x * PEN_SLICE;
    if (lo >= n) return;                                  // (workgroup-uniform; the launcher's grid never has such a slice)
    if (seq_rep) rep = seq_rep[b];
    if (seq_freq) freq = seq_freq[b];
    if (seq_pres) pres = seq_pres[b];
    if (rep == 1.f && freq == 0.f && pres == 0.f) return;   // 1. a neutral sequence (workgroup-uniform)
    const u32 width = (u32)((n - lo < PEN_SLICE ? n - lo : PEN_SLICE));
    int L = lengths[b];
    L = L < 0 ? 0 : L > cap ? cap : L;
    const int P = prompt_lens ? prompt_lens[b] : 0;

    for (int i = tid; i < PEN_SLICE / 4; i += PEN_THREADS) reinterpret_cast<v4u*>(s_cnt)[i] = v4u{0, 0, 0, 0};
    for (int i = tid; i < 3 * PEN_THREADS; i += PEN_THREADS) s_mark[i] = 0;
    if (tid < PEN_MAX_NODES) s_par[tid] = parents && tid < n_nodes ? parents[tid] : -1;
    __syncthreads();

    // ---- 2. the history, counted once
    const int* __restrict__ g_h = history + (size_t)b * hist_stride;
    auto count = [&](int t, int p) {
        const u32 d = (u32)t - (u32)lo;                   // (a negative id wraps far beyond any width: n <= 2^22)
        if (d < width) atomicAdd(&s_cnt[d], p >= P ? 0x10001u : 1u);
    };
    if ((reinterpret_cast<uintptr_t>(g_h) & 15) == 0) {   // (workgroup-uniform)
        const int quads = L >> 2;
        for (int q = tid; q < quads; q += PEN_THREADS) {
            const v4i v = reinterpret_cast<const v4i*>(g_h)[q];
            count(v[0], 4 * q);
            count(v[1], 4 * q + 1);
            count(v[2], 4 * q + 2);
            count(v[3], 4 * q + 3);
        }
        for (int p = 4 * quads + tid; p < L; p += PEN_THREADS) count(g_h[p], p);
    } else {
        for (int p = tid; p < L; p += PEN_THREADS) count(g_h[p], p);
    }
    if (tid == PEN_THREADS - 1) {                         // the path masks (s_par was written before the barrier above)
        s_anc[0] = 0;
        for (int i = 1; i < PEN_MAX_NODES; ++i) {
            const int a = s_par[i];
            s_anc[i] = i < n_nodes ? (1ull << i) | (a >= 1 && a < i ? s_anc[a] : 0ull) : 0ull;
        }
    }
    __syncthreads();

    // ---- 3. the owners' masks; wave 0: the nodes' tokens
    u32 nz = 0;
#pragma unroll
    for (int k = 0; k < PEN_OWNED; ++k) nz |= (s_cnt[tid + k * PEN_THREADS] != 0 ? 1u : 0u) << k;
    int loc = -1;                                         // wave 0, lane l: node l's id within the slice, -1 if it has none here
    u32 base = 0;
    u64 same = 0;
    if (wave == 0) {
        if (node_tokens && lane >= 1 && lane < n_nodes) {
            const long long t = node_tokens[(size_t)b * n_nodes + lane];
            if (t >= lo && t < (long long)lo + width) loc = (int)(t - lo);
        }
        if (loc >= 0) base = s_cnt[loc];
        for (int j = 1; j < PEN_MAX_NODES; ++j) same |= (u64)(__shfl(loc, j, 64) == loc ? 1 : 0) << j;
    }

    // ---- 4. the rows
    bool prev_mine = false;
    for (int i = 0; i < n_nodes; ++i) {
        u32* mark = s_mark + (i % 3) * PEN_THREADS;
        const u64 onp = s_anc[i];
        const bool mine = loc >= 0 && ((onp >> lane) & 1);    // (wave 0 only: loc is -1 elsewhere)
        if (mine) atomicOr(&mark[loc & (PEN_THREADS - 1)], 1u << (loc >> 10));
        __syncthreads();
        if (prev_mine) s_mark[((i + 2) % 3) * PEN_THREADS + (loc & (PEN_THREADS - 1))] = 0;   // row i - 1's marks
        prev_mine = mine;
        _Float16* row = logits + (size_t)((long long)b * n_nodes + i) * row_stride + lo;
        u32 m = nz & ~mark[tid];
        while (m) {
            const int idx = tid + (__builtin_ctz(m) << 10);
            m &= m - 1;
            edit(row + idx, s_cnt[idx], rep, freq, pres);
        }
        if (mine && (same & onp & ((1ull << lane) - 1)) == 0)
            edit(row + loc, base + (u32)__popcll(same & onp) * 0x10001u, rep, freq, pres);
    }
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

extern "C" int qs_penalize_rows(void* logits, int64_t row_stride, int n, const int32_t* history, int64_t hist_stride, int cap,
                                const int32_t* lengths, const int32_t* prompt_lens, const int64_t* node_tokens, const int32_t* parents,
                                int batch, int n_nodes, float repetition, float frequency, float presence, const float* seq_repetition,
                                const float* seq_frequency, const float* seq_presence, qs_stream_t stream) {
    QS_REQUIRE(logits && history && lengths, "penalize_rows: null pointer");
    QS_REQUIRE(!node_tokens || parents, "penalize_rows: node_tokens without parents");
    QS_REQUIRE(n >= 8 && n <= (1 << 22) && row_stride >= n && row_stride % 8 == 0,
               "penalize_rows: n=%d (8 .. 4194304), row stride %lld (must be >= n, multiple of 8)", n, (long long)row_stride);
    QS_REQUIRE(n_nodes >= 1 && n_nodes <= PEN_MAX_NODES, "penalize_rows: n_nodes=%d, a tree has 1 .. %d nodes", n_nodes, PEN_MAX_NODES);
    QS_REQUIRE(cap >= 1 && hist_stride >= cap, "penalize_rows: cap=%d, hist_stride=%lld (1 <= cap <= hist_stride)", cap,
               (long long)hist_stride);
    QS_REQUIRE(cap + (PEN_MAX_NODES - 1) <= PEN_MAX_COUNT, "penalize_rows: cap=%d, the 16-bit counts need cap + %d <= %d", cap,
               PEN_MAX_NODES - 1, PEN_MAX_COUNT);
    QS_REQUIRE(batch >= 0 && batch <= PEN_MAX_BATCH, "penalize_rows: batch=%d (0 .. %d: one grid row per sequence)", batch, PEN_MAX_BATCH);
    QS_REQUIRE(aligned(logits, 2) && aligned(node_tokens, 8), "penalize_rows: logits must be 2-byte, node_tokens 8-byte aligned");
    QS_REQUIRE(aligned(history, 4) && aligned(lengths, 4) && aligned(prompt_lens, 4) && aligned(parents, 4) && aligned(seq_repetition, 4) &&
                   aligned(seq_frequency, 4) && aligned(seq_presence, 4),
               "penalize_rows: the int32 and float arrays must be 4-byte aligned");
    if (batch == 0) return QS_OK;
    hipLaunchKernelGGL(penalize_rows_kernel, dim3((n + PEN_SLICE - 1) / PEN_SLICE, batch), dim3(PEN_THREADS), 0, (hipStream_t)stream,
                       (_Float16*)logits, (long long)row_stride, n, history, (long long)hist_stride, cap, lengths, prompt_lens,
                       (const long long*)node_tokens, parents, n_nodes, repetition, frequency, presence, seq_repetition, seq_frequency,
                       seq_presence);
    return qs_launch_status("penalize_rows");
}
