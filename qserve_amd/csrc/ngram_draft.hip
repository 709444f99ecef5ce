// ngram_draft.hip -- the drafter half of speculative decoding on the device, for MI355X (gfx950): prompt-lookup (n-gram) drafting of one
// token tree per sequence from the sequence's own token history, and the append that records what a verification accepted.  DESIGN.md 10
// ("N-gram drafting"); the rule is the header comment of qs_ngram_draft_tree / qs_history_append in include/qserve_amd.h.  (Its own
// translation unit: tree_accept.hip's set of three kernels is a checked contract.)  This file holds TWO kernels.
//
//   ngram_draft_tree_kernel  one workgroup of 1024 threads per sequence; no cross-workgroup communication, no waits, no scratch.
//              While L <= DRAFT_LDS_TOKENS the history h[0 .. L) is staged into LDS as int32; beyond it every read of h goes to global
//              memory (the row is L2-resident after the first node's scan).  The two paths are one body, draft_nodes, instantiated
//              with the reader of h: they differ in the address space of h alone.  The nodes are walked in index order (a parent is an
//              earlier node).  Per node:
//                1. wave 0 gathers the tokens of the node's earlier siblings - lane s keeps draft[s] in a register - into s_excl (one
//                   ballot, one prefix count);
//                2. every thread strides over the history positions p = 1 + tid, 1 + tid + 1024, ...: it compares h[p - 1] with the last
//                   context token (a register; rejects almost every p), extends the match backwards against the parent's context row in
//                   LDS (a broadcast read), and - only where the key (m << 32 | p) would beat its own best - checks h[p] against s_excl;
//                3. a wave max over the keys (six xor shuffles of two words), the 16 wave results through LDS, and every thread takes
//                   their maximum: p* is workgroup-uniform.  Thread 0 stores the token, threads 0 .. 15 write the node's context row:
//                   s_ctx[i] = draft[i] followed by the first 15 entries of the parent's row (the last 16 tokens of the node's c).
//              Two barriers per node.  A node whose parent entry is not in 0 .. i - 1 gets pad_token and the context row of a child of
//              the root (its path is the node alone).  Consecutive lanes read consecutive words of h: no LDS bank conflict.
//
//              Static LDS (the budget tests/test_ngram_draft_contracts.py holds the file to: DRAFT_LDS_BUDGET = 144 KiB of the CU's 160):
//              s_h 128 KiB + s_ctx 8 KiB + s_excl 512 B + s_red 128 B + s_par 256 B + one count.
//
//   history_append_kernel  thread (b, j), 1 <= j <= max_accept: history[b, past + j] = the token of the j-th accepted node (j < m) or the
//              bonus token (j == m); one 4-byte vector store, skipped at an index outside 0 .. cap - 1.
#include "common.h"

namespace {

constexpr int MAX_NODES = 64;                        // nodes per tree
constexpr int MAX_NGRAM = 16;                        // longest match looked for = tokens per context row
constexpr int DRAFT_THREADS = 1024;
constexpr int DRAFT_WAVES = DRAFT_THREADS / 64;
constexpr int DRAFT_LDS_TOKENS = 32768;              // history tokens staged in LDS (qserve_amd.drafting.LDS_TOKENS)
constexpr int DRAFT_LDS_BUDGET = 144 * 1024;         // bytes of static LDS the kernel may use

typedef unsigned long long u64;

__device__ __forceinline__ u64 wave_max_u64(u64 v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const u32 lo = (u32)__shfl_xor((int)(u32)v, o, 64), hi = (u32)__shfl_xor((int)(u32)(v >> 32), o, 64);
        const u64 w = ((u64)hi << 32) | lo;
        v = w > v ? w : v;
    }
    return v;
}

// The walk over the nodes of one sequence; `h` reads a history token (LDS or global), everything else is the workgroup's LDS.
template <class H>
__device__ __forceinline__ void draft_nodes(H h, int L, int n, int max_ngram, int min_match, long long pad_token, long long* __restrict__ out,
                                            long long* s_ctx, long long* s_excl, u64* s_red, const int* s_par, int* s_nexcl) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // node 0: the root, h[L - 1]; its context row is the tail of h
    const long long root = L > 0 ? (long long)h(L - 1) : pad_token;
    if (tid < MAX_NGRAM && tid < L) s_ctx[tid] = (long long)h(L - 1 - tid);
    if (tid == 0) out[0] = root;
    long long mine = root;                                // wave 0, lane s: draft[s] once node s is done (lane 0: the root)

    for (int i = 1; i < n; ++i) {
        const int a = s_par[i];
        const bool formed = a >= 0 && a < i;
        const int arow = formed ? a : 0;                  // (a malformed node reads the root's row: its path is the node alone)
        if (wave == 0) {                                  // 1. the exclusion list: earlier siblings' tokens, in index order
            const bool sib = formed && lane >= 1 && lane < i && s_par[lane] == a;
            const u64 votes = __ballot(sib);
            if (sib) s_excl[__popcll(votes & ((1ull << lane) - 1))] = mine;
            if (lane == 0) *s_nexcl = __popcll(votes);
        }
        __syncthreads();                                  // s_excl, s_nexcl; the context rows of the earlier iterations
        u64 best = 0;
        if (formed) {                                     // 2. the scan (workgroup-uniform branch)
            const long long* ctx = s_ctx + arow * MAX_NGRAM;
            const long long c0 = ctx[0];
            const int nexcl = *s_nexcl;
            for (int p = 1 + tid; p < L; p += DRAFT_THREADS) {
                if ((long long)h(p - 1) != c0) continue;
                const int lim = max_ngram < p ? max_ngram : p;
                int m = 1;
                while (m < lim && (long long)h(p - 1 - m) == ctx[m]) ++m;
                if (m < min_match) continue;
                const u64 key = ((u64)m << 32) | (u32)p;
                if (key <= best) continue;                // (p ascends: only a longer or equal match can still win)
                const long long t = (long long)h(p);
                bool unused = true;
                for (int s = 0; s < nexcl; ++s) unused = unused && s_excl[s] != t;
                if (unused) best = key;
            }
        }
        best = wave_max_u64(best);                        // 3. p* for the workgroup
        if (lane == 0) s_red[wave] = best;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < DRAFT_WAVES; ++w) best = s_red[w] > best ? s_red[w] : best;
        const long long tok = best ? (long long)h((int)(u32)best) : pad_token;
        if (tid == 0) out[i] = tok;
        if (tid == i) mine = tok;                         // (i < 64: a lane of wave 0)
        if (tid < MAX_NGRAM) s_ctx[i * MAX_NGRAM + tid] = tid == 0 ? tok : s_ctx[arow * MAX_NGRAM + tid - 1];
        // (the next iteration's first barrier orders these writes, and the reads of s_red above, before their next use)
    }
}

// grid = (sequences), 1024 threads.  n in 1 .. 64, 1 <= min_match <= max_ngram <= 16, cap >= 1, hist_stride >= cap (the launcher checks).
__global__ __launch_bounds__(DRAFT_THREADS) void ngram_draft_tree_kernel(const int* __restrict__ history, long long hist_stride, int cap,
                                                                          const int* __restrict__ lengths, const int* __restrict__ parents,
                                                                          int n, int max_ngram, int min_match, long long pad_token,
                                                                          long long* __restrict__ draft) {
    __shared__ int s_h[DRAFT_LDS_TOKENS];
    __shared__ long long s_ctx[MAX_NODES * MAX_NGRAM];   // row i: c[len(c) - 1 - j] of the children of node i, j < 16
    __shared__ long long s_excl[MAX_NODES];              // tokens of the node's earlier siblings
    __shared__ u64 s_red[DRAFT_WAVES];
    __shared__ int s_par[MAX_NODES];
    __shared__ int s_nexcl;
    static_assert(sizeof(s_h) + sizeof(s_ctx) + sizeof(s_excl) + sizeof(s_red) + sizeof(s_par) + sizeof(s_nexcl) <= DRAFT_LDS_BUDGET,
                  "static LDS beyond the documented budget");
    const int b = blockIdx.x, tid = threadIdx.x;
    int L = lengths[b];
    L = L < 0 ? 0 : L > cap ? cap : L;
    const int* __restrict__ g_h = history + (size_t)b * hist_stride;
    long long* out = draft + (size_t)b * n;
    if (tid < MAX_NODES) s_par[tid] = tid < n ? parents[tid] : -1;
    if (L <= DRAFT_LDS_TOKENS) {                         // (workgroup-uniform)
        for (int i = tid; i < L; i += DRAFT_THREADS) s_h[i] = g_h[i];
        __syncthreads();
        draft_nodes([&](int i) { return s_h[i]; }, L, n, max_ngram, min_match, pad_token, out, s_ctx, s_excl, s_red, s_par, &s_nexcl);
    } else {
        __syncthreads();
        draft_nodes([&](int i) { return g_h[i]; }, L, n, max_ngram, min_match, pad_token, out, s_ctx, s_excl, s_red, s_par, &s_nexcl);
    }
}

// grid = (sequences), 64 threads: thread -> j = 1 + its index (max_accept <= 64).
__global__ __launch_bounds__(64) void history_append_kernel(int* __restrict__ history, long long hist_stride, int cap,
                                                            const int* __restrict__ past_lens, const long long* __restrict__ node_tokens,
                                                            const int* __restrict__ accept_idx, const int* __restrict__ accept_lens,
                                                            const long long* __restrict__ next_token, int n, int max_accept) {
    const int b = blockIdx.x, j = 1 + threadIdx.x;
    int m = accept_lens[b];
    m = m > max_accept ? max_accept : m;
    if (m < 1 || j > m) return;
    long long val;
    if (j == m) {
        val = next_token[b];
    } else {
        const int idx = accept_idx[(size_t)b * max_accept + j];
        if (idx < 0 || idx >= n) return;                  // (no node of the tree: nothing to record)
        val = node_tokens[(size_t)b * n + idx];
    }
    const long long pos = (long long)past_lens[b] + j;
    if (pos < 0 || pos >= cap) return;
    history[(size_t)b * hist_stride + pos] = (int)val;
}

}  // namespace

extern "C" int qs_ngram_draft_tree(const int32_t* history, int64_t hist_stride, int cap, const int32_t* lengths, const int32_t* parents,
                                   int batch, int n, int max_ngram, int min_match, int64_t pad_token, int64_t* draft, qs_stream_t stream) {
    QS_REQUIRE(history && lengths && parents && draft, "ngram_draft_tree: null pointer");
    QS_REQUIRE(n >= 1 && n <= MAX_NODES, "ngram_draft_tree: n=%d, a tree has 1 .. %d nodes", n, MAX_NODES);
    QS_REQUIRE(max_ngram >= 1 && max_ngram <= MAX_NGRAM && min_match >= 1 && min_match <= max_ngram,
               "ngram_draft_tree: max_ngram=%d, min_match=%d (1 <= min_match <= max_ngram <= %d)", max_ngram, min_match, MAX_NGRAM);
    QS_REQUIRE(cap >= 1 && hist_stride >= cap, "ngram_draft_tree: cap=%d, hist_stride=%lld (1 <= cap <= hist_stride)", cap,
               (long long)hist_stride);
    QS_REQUIRE(batch >= 0, "ngram_draft_tree: batch=%d", batch);
    if (batch == 0) return QS_OK;
    hipLaunchKernelGGL(ngram_draft_tree_kernel, dim3(batch), dim3(DRAFT_THREADS), 0, (hipStream_t)stream, history, (long long)hist_stride, cap,
                       lengths, parents, n, max_ngram, min_match, (long long)pad_token, (long long*)draft);
    return qs_launch_status("ngram_draft_tree");
}

extern "C" int qs_ngram_draft_lds_tokens(void) { return DRAFT_LDS_TOKENS; }

extern "C" int qs_history_append(int32_t* history, int64_t hist_stride, int cap, const int32_t* past_lens, const int64_t* node_tokens,
                                 const int32_t* accept_idx, const int32_t* accept_lens, const int64_t* next_token, int batch, int n,
                                 int max_accept, qs_stream_t stream) {
    QS_REQUIRE(history && past_lens && node_tokens && accept_idx && accept_lens && next_token, "history_append: null pointer");
    QS_REQUIRE(n >= 1 && n <= MAX_NODES, "history_append: n=%d, a tree has 1 .. %d nodes", n, MAX_NODES);
    QS_REQUIRE(max_accept >= 1 && max_accept <= MAX_NODES, "history_append: max_accept=%d, a path has 1 .. %d nodes", max_accept, MAX_NODES);
    QS_REQUIRE(cap >= 1 && hist_stride >= cap, "history_append: cap=%d, hist_stride=%lld (1 <= cap <= hist_stride)", cap, (long long)hist_stride);
    QS_REQUIRE(batch >= 0, "history_append: batch=%d", batch);
    if (batch == 0) return QS_OK;
    hipLaunchKernelGGL(history_append_kernel, dim3(batch), dim3(64), 0, (hipStream_t)stream, history,
                       (long long)hist_stride, cap, past_lens, (const long long*)node_tokens, accept_idx, accept_lens,
                       (const long long*)next_token, n, max_accept);
    return qs_launch_status("history_append");
}
