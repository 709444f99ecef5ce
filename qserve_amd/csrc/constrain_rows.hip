// constrain_rows.hip -- constrained decoding on the device, for MI355X (gfx950): a token automaton (token_class int16 [n_vocab], next
// int32 [S, C]) masks fp16 logit rows in front of the sampling head (qs_argmax_rows / qs_sample_rows), behind the penalties, and one
// int32 per sequence follows the text through it.  DESIGN.md 10 ("Constrained decoding"); the rules are the header comments of
// qs_constrain_node_states / qs_constrain_rows / qs_constrain_advance in include/qserve_amd.h.  Everything is integer: bit-identical
// run to run and eager against graph replay.  No cross-workgroup communication, no waits, no scratch.  This file holds THREE kernels:
//
//   constrain_node_states_kernel  one wave64 per sequence, lane i = node i of the draft tree.  Every lane loads its token, its class and
//              its parent entry up front (independent loads); then the nodes are resolved in index order - a parent is an EARLIER node,
//              so its state is final when its child's turn comes - with one wave-uniform shuffle of the parent's state and one `next`
//              lookup in the node's own lane per step: only those lookups depend on each other.
//
//   constrain_rows_kernel  THE HOT ONE.  grid = (rows, slices of the vocabulary), 512 threads.  A workgroup whose row is unconstrained
//              leaves at once: nothing of the row is read or written.  Otherwise
//                1. the allowed set of the row's state is staged as a BITMASK, one bit per class - 4 KiB of LDS at the largest
//                   C = 32 768 instead of the 128 KiB the row itself would take, so the workgroups per CU are bounded by waves, not by
//                   LDS, at every C, and one instantiation serves all of them.  Wave w takes the groups g = w, w + 8, ... of 256
//                   classes: lane l loads next[s, 256 g + 4 l .. + 4) (one 16-byte load where the row is 16-byte aligned and the four
//                   lie below C, single loads below C otherwise; all of a wave's loads are issued before the first ballot), four
//                   ballots of `>= 0`, and lanes 0 .. 3 store the 64 bits of one ballot each.  The layout is the ballots': class c sits
//                   in 64-bit word 4 (c / 256) + c % 4 at bit (c / 4) % 64;
//                2. per lane 16-byte loads of 8 logits and of 8 classes, one 4-byte LDS read per class (a class outside 0 .. C-1 reads
//                   word 0 and is refused by the range test: no address is formed from it), a blend with 0xFC00, and a 16-byte store
//                   only where a bit changed.  The last n_vocab % 8 ids of a row are edited one by one: the padding behind n_vocab is
//                   neither read nor written.
//              The launcher cuts a row into min(chunks, max(n_vocab / 4 C, 1024 / rows)) slices (both quotients rounded up; a chunk
//              is the 4096 ids of one pass): as fine as keeps staging (4 C bytes of `next`, cache hits) below a quarter of the slice's
//              own traffic, or finer where that is what 1024 workgroups take.  One chunk per workgroup wherever C <= 1024 or the rows
//              are few (a decode step); several passes per workgroup only at C > 1024 with rows enough.
//
//   constrain_advance_kernel  one thread per sequence: the state of the row that emitted the round's last token, moved over that token.
#include "common.h"

namespace {

constexpr int CR_THREADS = 512;
constexpr int CR_WAVES = CR_THREADS / 64;
constexpr int CR_CHUNK = CR_THREADS * 8;             // logits one pass of a workgroup covers; slices are multiples of it
constexpr int CR_MAX_CLASSES = 32768;
constexpr int CR_STAGE = 4;                          // groups of 256 classes a wave loads before it ballots
constexpr int CR_MIN_WORKGROUPS = 1024;              // what the launcher cuts a small launch into, where the rows are long enough
constexpr int CR_MAX_NODES = 64;
constexpr int CR_MAX_ROWS = 1 << 24;                 // rows / sequences per launch (the grid's x extent is far beyond it)
constexpr int ADV_THREADS = 256;
constexpr u32 NEG_INF_H = 0xFC00u;

typedef unsigned long long u64;

// the state behind `st` (in 0 .. S-1) over a token of class `cls` (-1: the token is out of the vocabulary or its class out of range)
__device__ __forceinline__ int move(int st, int cls, const int* __restrict__ next, long long next_stride) {
    if (cls < 0) return QS_FSM_DEAD;
    const int v = next[(size_t)st * next_stride + cls];
    return v < 0 ? QS_FSM_DEAD : v;
}

// the class of token t, -1 where t is outside [0, n_vocab) or its class outside [0, C): nothing is read for an id out of range
__device__ __forceinline__ int class_of(long long t, const short* __restrict__ token_class, int n_vocab, int C) {
    if (t < 0 || t >= n_vocab) return -1;
    const int c = token_class[t];
    return c >= C ? -1 : c;
}

// grid = sequences, 64 threads.  The launcher checks n.
__global__ __launch_bounds__(64) void constrain_node_states_kernel(const int* __restrict__ state, const long long* __restrict__ node_tokens,
                                                                   const int* __restrict__ parents, const short* __restrict__ token_class,
                                                                   int n_vocab, const int* __restrict__ next, long long next_stride, int S,
                                                                   int C, int n, int* __restrict__ node_state) {
    const int b = blockIdx.x, lane = threadIdx.x;
    int cls = -1, par = 0;
    if (lane >= 1 && lane < n) {
        cls = class_of(node_tokens[(size_t)b * n + lane], token_class, n_vocab, C);
        par = parents[lane];
    }
    int st = state[b];                                    // lane 0: the root's; every other lane's is replaced at its turn
    for (int i = 1; i < n; ++i) {                         // (wave-uniform: both shuffles run with all 64 lanes)
        int a = __shfl(par, i, 64);
        a = a >= 0 && a < i ? a : 0;                      // a malformed entry hangs the node off the root
        const int pst = __shfl(st, a, 64);
        if (lane == i) st = pst < 0 || pst >= S ? pst : move(pst, cls, next, next_stride);
    }
    if (lane < n) node_state[(size_t)b * n + lane] = st;
}

// one logit under the mask: its bits where class c is allowed, -inf otherwise.  Class c: 64-bit word 4 (c / 256) + c % 4, bit (c / 4) % 64
__device__ __forceinline__ u32 blend(u32 bits, int c, int C, const u32* s_ok) {
    const bool in = (u32)c < (u32)C;
    const u32 cc = in ? (u32)c : 0u;
    const u32 w = s_ok[(((cc >> 8) << 2) | (cc & 3u)) << 1 | ((cc >> 7) & 1u)];
    return in && ((w >> ((cc >> 2) & 31u)) & 1u) ? bits : NEG_INF_H;
}

// grid = (rows, slices), 512 threads; `slice` ids per workgroup, a multiple of CR_CHUNK.  The launcher checks the strides and C.
__global__ __launch_bounds__(CR_THREADS) void constrain_rows_kernel(_Float16* __restrict__ logits, long long row_stride, int n_vocab,
                                                                    const int* __restrict__ row_state,
                                                                    const short* __restrict__ token_class, const int* __restrict__ next,
                                                                    long long next_stride, int S, int C, int slice) {
    __shared__ __attribute__((aligned(16))) u32 s_ok[CR_MAX_CLASSES / 32];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long lo64 = (long long)blockIdx.y * slice;
    const int s = row_state[r];
    if (s < 0 || s >= S || lo64 >= n_vocab) return;      // an unconstrained row (workgroup-uniform; the grid never has such a slice)
    const int lo = (int)lo64;

    // ---- 1. the allowed classes of state s, one bit each
    const int* __restrict__ nrow = next + (size_t)s * next_stride;
    const bool vec = (reinterpret_cast<uintptr_t>(nrow) & 15) == 0;          // (workgroup-uniform)
    const int groups = (C + 255) >> 8;
    for (int g0 = wave; g0 < groups; g0 += CR_STAGE * CR_WAVES) {            // (wave-uniform: the ballots run with all 64 lanes)
        v4i v[CR_STAGE];
#pragma unroll
        for (int u = 0; u < CR_STAGE; ++u) {                                  // the loads of CR_STAGE groups, then their ballots
            const int c = (g0 + u * CR_WAVES) * 256 + lane * 4;               // (a group beyond the last: c >= C, nothing is read)
            if (vec && c + 3 < C) {
                v[u] = *reinterpret_cast<const v4i*>(nrow + c);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) v[u][j] = c + j < C ? nrow[c + j] : -1;
            }
        }
#pragma unroll
        for (int u = 0; u < CR_STAGE; ++u) {
            const int g = g0 + u * CR_WAVES;
            u64 m = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const u64 bj = __ballot(v[u][j] >= 0);
                m = lane == j ? bj : m;
            }
            if (g < groups && lane < 4) *reinterpret_cast<v2u*>(&s_ok[(g * 4 + lane) * 2]) = v2u{(u32)m, (u32)(m >> 32)};
        }
    }
    __syncthreads();

    // ---- 2. the slice, 8 ids per lane and pass
    const int hi = n_vocab - lo < slice ? n_vocab : lo + slice;
    const int full = lo + ((hi - lo) & ~7);               // whole vectors end here; lo is a multiple of 8
    _Float16* __restrict__ row = logits + (size_t)r * row_stride;
#pragma unroll 2
    for (int t = lo + tid * 8; t < full; t += CR_CHUNK) {
        const v4u x = *reinterpret_cast<const v4u*>(row + t);
        const v4u k = *reinterpret_cast<const v4u*>(token_class + t);
        v4u y;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const u32 a = blend(x[j] & 0xFFFFu, (int)(short)(k[j] & 0xFFFFu), C, s_ok);
            const u32 b = blend(x[j] >> 16, (int)(short)(k[j] >> 16), C, s_ok);
            y[j] = a | (b << 16);
        }
        if (((y[0] ^ x[0]) | (y[1] ^ x[1]) | (y[2] ^ x[2]) | (y[3] ^ x[3])) != 0) *reinterpret_cast<v4u*>(row + t) = y;
    }
    if (tid < hi - full) {                                // the last n_vocab % 8 ids (of the last slice only)
        unsigned short* p = reinterpret_cast<unsigned short*>(row) + full + tid;
        const u32 x = *p, y = blend(x, (int)token_class[full + tid], C, s_ok);
        if (y != x) *p = (unsigned short)y;
    }
}

// grid = ceil(batch / 256), 256 threads: one thread per sequence.  The launcher checks n and max_accept.
__global__ __launch_bounds__(ADV_THREADS) void constrain_advance_kernel(int* __restrict__ state, const int* __restrict__ node_state,
                                                                        const int* __restrict__ accept_idx,
                                                                        const int* __restrict__ accept_lens,
                                                                        const long long* __restrict__ next_token,
                                                                        const short* __restrict__ token_class, int n_vocab,
                                                                        const int* __restrict__ next, long long next_stride, int S, int C,
                                                                        int batch, int n, int max_accept) {
    const int b = blockIdx.x * ADV_THREADS + threadIdx.x;
    if (b >= batch) return;
    int k = accept_lens ? accept_lens[b] : 1;
    k = k < 0 ? 0 : k > max_accept ? max_accept : k;
    if (k == 0) return;                                   // a frozen row, or a path clipped to nothing
    int st;
    if (node_state && accept_idx) {
        int i = accept_idx[(size_t)b * max_accept + (k - 1)];
        i = i < 0 ? 0 : i > n - 1 ? n - 1 : i;
        st = node_state[(size_t)b * n + i];
    } else {
        st = state[b];
    }
    if (st < 0 || st >= S) return;                        // unconstrained, or dead
    state[b] = move(st, class_of(next_token[b], token_class, n_vocab, C), next, next_stride);
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// what the three entries ask of the tables
#define QS_REQUIRE_TABLES(what)                                                                                                         \
    QS_REQUIRE(n_vocab >= 8 && n_vocab <= (1 << 22), what ": n_vocab=%d (8 .. 4194304)", n_vocab);                                     \
    QS_REQUIRE(C >= 1 && C <= CR_MAX_CLASSES && S >= 1 && next_stride >= C,                                                              \
               what ": C=%d (1 .. %d), S=%d (>= 1), next_stride=%lld (>= C)", C, CR_MAX_CLASSES, S, (long long)next_stride);             \
    QS_REQUIRE(aligned(token_class, 16) && aligned(next, 4), what ": token_class must be 16-byte, next 4-byte aligned")

}  // namespace

extern "C" int qs_constrain_node_states(const int32_t* state, const int64_t* node_tokens, const int32_t* parents, const int16_t* token_class,
                                        int n_vocab, const int32_t* next, int64_t next_stride, int S, int C, int batch, int n,
                                        int32_t* node_state, qs_stream_t stream) {
    QS_REQUIRE(state && token_class && next && node_state, "constrain_node_states: null pointer");
    QS_REQUIRE(n >= 1 && n <= CR_MAX_NODES, "constrain_node_states: n=%d, a tree has 1 .. %d nodes", n, CR_MAX_NODES);
    QS_REQUIRE(n == 1 || (node_tokens && parents), "constrain_node_states: n=%d > 1 needs node_tokens and parents", n);
    QS_REQUIRE_TABLES("constrain_node_states");
    QS_REQUIRE(batch >= 0 && batch <= CR_MAX_ROWS, "constrain_node_states: batch=%d (0 .. %d)", batch, CR_MAX_ROWS);
    QS_REQUIRE(aligned(node_tokens, 8) && aligned(state, 4) && aligned(parents, 4) && aligned(node_state, 4),
               "constrain_node_states: node_tokens must be 8-byte, the int32 arrays 4-byte aligned");
    if (batch == 0) return QS_OK;
    hipLaunchKernelGGL(constrain_node_states_kernel, dim3(batch), dim3(64), 0, (hipStream_t)stream, state, (const long long*)node_tokens,
                       parents, token_class, n_vocab, next, (long long)next_stride, S, C, n, node_state);
    return qs_launch_status("constrain_node_states");
}

extern "C" int qs_constrain_rows(void* logits, int64_t row_stride, int n_vocab, const int32_t* row_state, const int16_t* token_class,
                                 const int32_t* next, int64_t next_stride, int S, int C, int rows, qs_stream_t stream) {
    QS_REQUIRE(logits && row_state && token_class && next, "constrain_rows: null pointer");
    QS_REQUIRE_TABLES("constrain_rows");
    QS_REQUIRE(row_stride >= n_vocab && row_stride % 8 == 0, "constrain_rows: row stride %lld (must be >= n_vocab=%d, multiple of 8)",
               (long long)row_stride, n_vocab);
    QS_REQUIRE(rows >= 0 && rows <= CR_MAX_ROWS, "constrain_rows: rows=%d (0 .. %d)", rows, CR_MAX_ROWS);
    QS_REQUIRE(aligned(logits, 16) && aligned(row_state, 4), "constrain_rows: logits must be 16-byte, row_state 4-byte aligned");
    if (rows == 0) return QS_OK;
    // a workgroup stages 4 C bytes of `next` (read by every workgroup of the row's state: cache hits) and moves 4 bytes per id of its
    // slice (logit + class).  Slices per row wanted = min(chunks, max(ceil(n_vocab / 4 C), ceil(CR_MIN_WORKGROUPS / rows))): the first
    // term is the finest cut that keeps a slice at >= 4 C ids, the staging below a quarter of the slice's traffic; the second asks for
    // CR_MIN_WORKGROUPS workgroups whatever the staging costs.  Hence a slice is ONE chunk wherever C <= 1024 (4 C <= CR_CHUNK), at any
    // row count, and wherever rows <= CR_MIN_WORKGROUPS / chunks (a decode step); it spans several chunks only where C > 1024 and
    // there are rows enough (a verification at a large C)
    const int chunks = (n_vocab + CR_CHUNK - 1) / CR_CHUNK;
    const int by_staging = (int)((n_vocab + 4ll * C - 1) / (4ll * C));
    const int by_rows = (CR_MIN_WORKGROUPS + rows - 1) / rows;
    int slices_wanted = by_staging > by_rows ? by_staging : by_rows;
    slices_wanted = slices_wanted > chunks ? chunks : slices_wanted;
    const int slice = ((chunks + slices_wanted - 1) / slices_wanted) * CR_CHUNK;
    const int slices = (n_vocab + slice - 1) / slice;
    hipLaunchKernelGGL(constrain_rows_kernel, dim3(rows, slices), dim3(CR_THREADS), 0, (hipStream_t)stream, (_Float16*)logits,
                       (long long)row_stride, n_vocab, row_state, token_class, next, (long long)next_stride, S, C, slice);
    return qs_launch_status("constrain_rows");
}

extern "C" int qs_constrain_advance(int32_t* state, const int32_t* node_state, const int32_t* accept_idx, const int32_t* accept_lens,
                                    const int64_t* next_token, const int16_t* token_class, int n_vocab, const int32_t* next,
                                    int64_t next_stride, int S, int C, int batch, int n, int max_accept, qs_stream_t stream) {
    QS_REQUIRE(state && next_token && token_class && next, "constrain_advance: null pointer");
    QS_REQUIRE(n >= 1 && n <= CR_MAX_NODES && max_accept >= 1 && max_accept <= CR_MAX_NODES,
               "constrain_advance: n=%d, max_accept=%d (1 .. %d each)", n, max_accept, CR_MAX_NODES);
    QS_REQUIRE(max_accept == 1 || accept_idx, "constrain_advance: max_accept=%d > 1 needs accept_idx", max_accept);
    QS_REQUIRE_TABLES("constrain_advance");
    QS_REQUIRE(batch >= 0 && batch <= CR_MAX_ROWS, "constrain_advance: batch=%d (0 .. %d)", batch, CR_MAX_ROWS);
    QS_REQUIRE(aligned(next_token, 8) && aligned(state, 4) && aligned(node_state, 4) && aligned(accept_idx, 4) && aligned(accept_lens, 4),
               "constrain_advance: next_token must be 8-byte, the int32 arrays 4-byte aligned");
    if (batch == 0) return QS_OK;
    hipLaunchKernelGGL(constrain_advance_kernel, dim3((batch + ADV_THREADS - 1) / ADV_THREADS), dim3(ADV_THREADS), 0, (hipStream_t)stream,
                       state, node_state, accept_idx, accept_lens, (const long long*)next_token, token_class, n_vocab, next,
                       (long long)next_stride, S, C, batch, n, max_accept);
    return qs_launch_status("constrain_advance");
}
