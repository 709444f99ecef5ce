// stop_update.hip -- the device-side stop rule of the decode loop, for MI355X (gfx950): stop sequences, length limits and frozen rows,
// applied to what one round (a decode step or a tree verification) is about to emit, between the walk and the commit.  DESIGN.md 10
// ("Stop conditions"); the rule is the header comment of qs_stop_update in include/qserve_amd.h, in exact integers.  This file
// holds ONE kernel.
//
//   stop_update_kernel  one wave64 per sequence, STOP_WAVES waves per workgroup; no LDS, no barrier, no cross-workgroup traffic, no
//              scratch.  Lane j owns the emitted index j (0: the current token, 1 .. m: e_1 .. e_m; a path of 64 nodes has a 65th
//              index, which lane 0 owns in a second pass that runs for m == 64 alone).
//                1. lane j loads e_j (the j-th accepted node's token, or the bonus token at j == m) into a register;
//                2. it builds the window of the 8 text positions that end at L - 1 + j: positions < L from `history`, later ones
//                   from the other lanes' registers (one 64-bit shuffle each), with one validity bit per position (inside the
//                   generated text and the history's capacity);
//                3. it compares the window's tail with every row of the stop table that is on and tests the length limit.  Which rows
//                   are on is one vector load (lane s: stop_lens[s]) and one ballot; the loop runs over the set bits alone, so an
//                   empty table costs no iteration, and a row's ids are read at wave-uniform addresses;
//                4. one 64-bit ballot of the hits, find-first-set: k; a second ballot of the stop hits gives the reason at k;
//                5. lane 0 writes accept_lens, finished, next_token and last_row (vector stores).
//              Every index is clamped before an address is formed from it: lengths to 0 .. cap, accept_idx entries to 0 .. n - 1.
#include "common.h"

namespace {

constexpr int MAX_NODES = 64;                        // nodes per tree, hence emitted tokens per round
constexpr int MAX_STOPS = 32;                        // rows of the stop table (qserve_amd.stopping.MAX_STOPS)
constexpr int MAX_STOP_LEN = 8;                      // tokens per row (qserve_amd.stopping.MAX_STOP_LEN)
constexpr int STOP_WAVES = 4;                        // sequences per workgroup

typedef unsigned long long u64;

struct StopArgs {
    const int* history;                              // [batch, cap], row stride hist_stride
    long long hist_stride;
    int cap;
    const int* lengths;                              // [batch], from before the round advanced them
    const int* prompt_lens;                          // [batch] or null
    const long long* node_tokens;                    // [batch, n] or null (n == 1)
    const int* accept_idx;                           // [batch, max_accept] or null (max_accept == 1)
    int* accept_lens;                                // [batch] in / out, or null (m = 1)
    int* out_lens;                                   // [batch], written when accept_lens is null
    long long* next_token;                           // [batch] in / out
    long long* last_row;                             // [batch] or null
    const int* stop_seqs;                            // [S, W]
    const int* stop_lens;                            // [S]
    const int* limit_lens;                           // [batch] or null
    int* finished;                                   // [batch] in / out
    int batch, n, max_accept, S, W, check_root;
};

__device__ __forceinline__ int clamp_node(int idx, int n) { return idx < 0 ? 0 : idx >= n ? n - 1 : idx; }

// hit(j) of this lane's index j; `stop`: case (b) holds at j.  Every lane of the wave calls it (it shuffles).  e: this lane's e_lane
// (lanes 1 .. min(m, 63)); bonus: e_m.
// rows: the table rows whose length is in 1 .. W, one bit each.
__device__ __forceinline__ bool stop_hit(const StopArgs& a, const int* __restrict__ h, int L, int m, int plen, bool limited, int limit,
                                         u64 rows, int j, long long e, long long bonus, bool& stop) {
    const bool mine = j <= m;
    const long long pend = (long long)L - 1 + j;     // the text position index j holds
    long long win[MAX_STOP_LEN];                     // win[u]: the token at position pend - u
    unsigned valid = 0;
#pragma unroll
    for (int u = 0; u < MAX_STOP_LEN; ++u) {
        const long long p = pend - u;
        const int jj = j - u;                        // the emitted index at p, where p >= L (then 1 <= jj <= m)
        const long long em = __shfl(e, jj < 0 ? 0 : jj & 63, 64);
        const bool ok = mine && p >= plen && p >= 0 && p < a.cap;
        const long long ph = p < 0 ? 0 : p >= a.cap ? a.cap - 1 : p;       // (every lane loads, from inside the row: no divergent load)
        const long long hv = (long long)h[ph];
        win[u] = p < L ? hv : jj == m ? bonus : em;                         // (read only where `ok`)
        valid |= (unsigned)ok << u;
    }
    bool any = false;
    for (u64 r = rows; r; r &= r - 1) {              // (wave-uniform: the rows that are on)
        const int s = __ffsll(r) - 1;
        const int len = a.stop_lens[s];
        bool match = true;
#pragma unroll
        for (int u = 0; u < MAX_STOP_LEN; ++u) {
            if (u < len) {
                const int id = a.stop_seqs[s * a.W + len - 1 - u];
                match = match && id >= 0 && ((valid >> u) & 1u) && win[u] == (long long)id;
            }
        }
        any = any || match;
    }
    stop = mine && any && j >= (a.check_root ? 0 : 1);
    return stop || (mine && limited && (long long)L + j >= (long long)limit);
}

// grid = ceil(batch / STOP_WAVES), STOP_WAVES * 64 threads.  1 <= n, max_accept <= 64, 0 <= S <= 32, 1 <= W <= 8, cap >= 1 (the launcher).
__global__ __launch_bounds__(STOP_WAVES * 64) void stop_update_kernel(const StopArgs a) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * STOP_WAVES + (threadIdx.x >> 6);
    if (b >= a.batch) return;                        // (wave-uniform)
    int L = a.lengths[b];
    L = L < 0 ? 0 : L > a.cap ? a.cap : L;
    int mcap = a.max_accept < MAX_NODES ? a.max_accept : MAX_NODES;
    if (!a.node_tokens || !a.accept_idx) mcap = 1;   // (a plain step: nothing but the bonus token can be emitted)
    int m = a.accept_lens ? a.accept_lens[b] : 1;
    m = m < 0 ? 0 : m > mcap ? mcap : m;
    const int plen = a.prompt_lens ? a.prompt_lens[b] : 0;
    const bool limited = a.limit_lens != nullptr;
    const int limit = limited ? a.limit_lens[b] : 0;
    const int fin = a.finished[b];
    const int* __restrict__ h = a.history + (size_t)b * a.hist_stride;
    const size_t idx_row = (size_t)b * a.max_accept, tok_row = (size_t)b * a.n;

    const long long bonus = a.next_token[b];
    long long e = 0;                                 // e_lane
    if (lane >= 1 && lane < m) e = a.node_tokens[tok_row + clamp_node(a.accept_idx[idx_row + lane], a.n)];
    if (lane == m) e = bonus;

    const int row_len = lane < a.S ? a.stop_lens[lane] : 0;                 // (S <= 32 < 64 lanes)
    const u64 rows = __ballot(row_len >= 1 && row_len <= a.W);

    int k = m, reason = 0;
    bool stop;
    const bool hit = stop_hit(a, h, L, m, plen, limited, limit, rows, lane, e, bonus, stop);
    const u64 hits = __ballot(hit), stops = __ballot(stop);
    if (hits) {
        k = __ffsll(hits) - 1;
        reason = ((stops >> k) & 1ull) ? 1 : 2;
    } else if (m == MAX_NODES) {                     // (wave-uniform) the 65th index: lane 0 holds j = 64, the others j > m
        const bool hit64 = stop_hit(a, h, L, m, plen, limited, limit, rows, MAX_NODES + lane, e, bonus, stop);
        const u64 hits64 = __ballot(hit64), stops64 = __ballot(stop);
        if (hits64 & 1ull) {
            k = MAX_NODES;
            reason = (stops64 & 1ull) ? 1 : 2;
        }
    }
    if (fin != 0) k = 0;                             // a finished row emits nothing; its reason stays
    const long long ek = __shfl(e, k & 63, 64);      // e_k, for 1 <= k < m <= 64
    if (lane != 0) return;
    (a.accept_lens ? a.accept_lens : a.out_lens)[b] = k;
    if (fin == 0 && reason != 0) a.finished[b] = reason;
    if (k == m) return;                              // the round emits all it was about to: next_token and last_row stay
    if (k >= 1) {
        a.next_token[b] = ek;
        if (a.last_row) a.last_row[b] = (long long)b * a.n + clamp_node(a.accept_idx[idx_row + k - 1], a.n);
    } else if (L >= 1) {                             // k == 0: the frozen token (L <= cap: the index is inside the row)
        a.next_token[b] = (long long)h[L - 1];
    }
}

}  // namespace

extern "C" int qs_stop_update(const int32_t* history, int64_t hist_stride, int cap, const int32_t* lengths, const int32_t* prompt_lens,
                              const int64_t* node_tokens, const int32_t* accept_idx, int32_t* accept_lens, int32_t* out_lens,
                              int64_t* next_token, int64_t* last_row, const int32_t* stop_seqs, const int32_t* stop_lens,
                              const int32_t* limit_lens, int32_t* finished, int batch, int n, int max_accept, int num_stops,
                              int stop_width, int check_root, qs_stream_t stream) {
    QS_REQUIRE(history && lengths && next_token && finished, "stop_update: null pointer");
    QS_REQUIRE(accept_lens || out_lens, "stop_update: null pointer (accept_lens is null: out_lens takes the result)");
    QS_REQUIRE(n >= 1 && n <= MAX_NODES, "stop_update: n=%d, a tree has 1 .. %d nodes", n, MAX_NODES);
    QS_REQUIRE(max_accept >= 1 && max_accept <= MAX_NODES, "stop_update: max_accept=%d, a path has 1 .. %d nodes", max_accept, MAX_NODES);
    QS_REQUIRE(num_stops >= 0 && num_stops <= MAX_STOPS, "stop_update: num_stops=%d (0 .. %d)", num_stops, MAX_STOPS);
    QS_REQUIRE(stop_width >= 1 && stop_width <= MAX_STOP_LEN, "stop_update: stop_width=%d (1 .. %d)", stop_width, MAX_STOP_LEN);
    QS_REQUIRE(num_stops == 0 || (stop_seqs && stop_lens), "stop_update: null pointer (num_stops=%d needs stop_seqs and stop_lens)", num_stops);
    QS_REQUIRE(node_tokens || n == 1, "stop_update: node_tokens is null with n=%d (only a plain step, n = 1, has no draft)", n);
    QS_REQUIRE(accept_idx || max_accept == 1, "stop_update: accept_idx is null with max_accept=%d", max_accept);
    QS_REQUIRE(cap >= 1 && hist_stride >= cap, "stop_update: cap=%d, hist_stride=%lld (1 <= cap <= hist_stride)", cap, (long long)hist_stride);
    QS_REQUIRE(check_root == 0 || check_root == 1, "stop_update: check_root=%d (0 / 1)", check_root);
    QS_REQUIRE(batch >= 0, "stop_update: batch=%d", batch);
    const uintptr_t words = (uintptr_t)history | (uintptr_t)lengths | (uintptr_t)prompt_lens | (uintptr_t)accept_idx | (uintptr_t)accept_lens |
                            (uintptr_t)out_lens | (uintptr_t)stop_seqs | (uintptr_t)stop_lens | (uintptr_t)limit_lens | (uintptr_t)finished;
    QS_REQUIRE((words & 3) == 0, "stop_update: an int32 array is not 4-byte aligned");
    QS_REQUIRE((((uintptr_t)node_tokens | (uintptr_t)next_token | (uintptr_t)last_row) & 7) == 0,
               "stop_update: node_tokens, next_token and last_row must be 8-byte aligned");
    if (batch == 0) return QS_OK;
    StopArgs a;
    a.history = history, a.hist_stride = (long long)hist_stride, a.cap = cap;
    a.lengths = lengths, a.prompt_lens = prompt_lens;
    a.node_tokens = (const long long*)node_tokens, a.accept_idx = accept_idx, a.accept_lens = accept_lens, a.out_lens = out_lens;
    a.next_token = (long long*)next_token, a.last_row = (long long*)last_row;
    a.stop_seqs = stop_seqs, a.stop_lens = stop_lens, a.limit_lens = limit_lens, a.finished = finished;
    a.batch = batch, a.n = n, a.max_accept = max_accept, a.S = num_stops, a.W = stop_width, a.check_root = check_root;
    hipLaunchKernelGGL(stop_update_kernel, dim3((batch + STOP_WAVES - 1) / STOP_WAVES), dim3(STOP_WAVES * 64), 0, (hipStream_t)stream, a);
    return qs_launch_status("stop_update");
}
