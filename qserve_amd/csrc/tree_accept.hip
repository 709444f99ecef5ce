// tree_accept.hip -- the tail of tree-draft verification on the device, for MI355X (gfx950): what DecodeEngine.verify_tree did on the host
// between the forward pass and the next step.  DESIGN.md 10 ("Tree verification").  (Its own translation unit: append_tree.hip's set of six
// kernels is a checked contract.)
//
//   tree_accept_greedy_kernel  the greedy walk.  One wave64 per sequence, lane j = node j with its parent and token in registers.  Node 0 is
//              accepted; from the current node `cur` the next one is the LOWEST c with cur < c < n, parents[c] == cur and
//              tokens[c] == argmax[cur] - one ballot and one find-first-set per level; the walk ends when no lane votes or the path holds
//              max_accept nodes.  Only c > cur is a candidate, so the walk increases strictly whatever `parents` holds (p >= i, p < -1,
//              self-loops): at most n levels, nothing outside the sequence's rows is read, no validation pass.  The loop is wave-uniform;
//              lane k keeps path[k] and the row of accept_idx leaves as one vector store, zeros behind the path.  No LDS, no scratch.
//
//   kv_commit_path_layers_kernel<DHB>  kv_commit_path_kernel (append_tree.hip) with the layer next to K | V in the grid: one launch moves
//              the accepted path in every layer.  layer_tables[l] is the device address of layer l's kv_pointers [batch, 2, max_blocks];
//              per (layer, K | V, KV head, sequence) the moves are kv_commit.h's - the one rule both kernels share.
#include "kv_commit.h"

namespace {

using namespace qs_commit;

// grid = (sequences), 64 threads.  n is cut to 64 nodes and to the rows the buffers hold (num_tokens), so every read is in bounds whatever
// cu_seqlens_q holds.
__global__ __launch_bounds__(64) void tree_accept_greedy_kernel(const int64_t* __restrict__ tokens, const int64_t* __restrict__ argmax,
                                                                const int* __restrict__ parents, const int* __restrict__ cu_q, int num_tokens,
                                                                int max_accept, int* __restrict__ accept_idx, int* __restrict__ accept_lens,
                                                                int64_t* __restrict__ last_row, int64_t* __restrict__ next_token) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int q0 = cu_q[b];
    int n = cu_q[b + 1] - q0;
    n = n > MAX_PATH ? MAX_PATH : n;
    if (q0 < 0 || q0 > num_tokens) n = 0;
    else if (n > num_tokens - q0) n = num_tokens - q0;
    const bool live = lane < n;
    const int par = live ? parents[q0 + lane] : -2;
    const long long tok = live ? (long long)tokens[q0 + lane] : 0;
    const long long am = live ? (long long)argmax[q0 + lane] : 0;
    const u32 am_lo = (u32)am, am_hi = (u32)((unsigned long long)am >> 32);
    auto argmax_at = [&](int node) {                      // argmax of a (wave-uniform) node: two lane reads, no LDS
        return (long long)(((unsigned long long)(u32)__builtin_amdgcn_readlane((int)am_hi, node) << 32) |
                           (u32)__builtin_amdgcn_readlane((int)am_lo, node));
    };
    int len = 0, cur = 0, mine = 0;                       // mine: path[lane] (0 behind the path - what the host loop padded with)
    if (n >= 1) {
        len = 1;                                          // the root: path[0] = 0 = `mine` of lane 0
        while (len < max_accept) {
            const long long want = argmax_at(cur);
            const unsigned long long votes = __ballot(live && lane > cur && par == cur && tok == want);
            if (votes == 0) break;
            cur = __ffsll(votes) - 1;                     // the lowest matching child
            if (lane == len) mine = cur;
            ++len;
        }
    }
    if (lane < max_accept) accept_idx[(size_t)b * max_accept + lane] = mine;
    if (lane == 0) accept_lens[b] = len;
    const long long want = argmax_at(cur);
    if (lane == 0) {
        if (last_row) last_row[b] = n >= 1 ? (int64_t)q0 + cur : -1;
        if (next_token && n >= 1) next_token[b] = want;
    }
}

// grid = (KV heads, 2 * layers: layer = y / 2, K | V = y % 2, sequences), 256 threads.
template <int DHB>
__global__ __launch_bounds__(256) void kv_commit_path_layers_kernel(const int64_t* __restrict__ layer_tables, const int* __restrict__ past_lens,
                                                                    const int* __restrict__ accept_idx, const int* __restrict__ accept_lens,
                                                                    int max_accept, int max_blocks, int kv_head_num) {
    constexpr int CH = DHB / 16;                         // 16-byte chunks per token
    __shared__ v4u s_data[MAX_PATH * CH];
    __shared__ u32 s_par[MAX_PATH];                      // (scale, zero) as two fp16
    const int hkv = blockIdx.x, layer = blockIdx.y >> 1, which = blockIdx.y & 1, b = blockIdx.z;
    int m = accept_lens[b];
    m = m < 0 ? 0 : m > max_accept ? max_accept : m;
    const int past = past_lens[b];
    const int64_t* kv_pointers = reinterpret_cast<const int64_t*>(layer_tables[layer]);
    const int64_t* tab = kv_pointers + ((size_t)b * 2 + which) * max_blocks;
    const int* idx = accept_idx + (size_t)b * max_accept;
    commit_path_moves<DHB>(tab, idx, m, past, hkv, max_blocks, kv_head_num, s_data, s_par);
}

inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

}  // namespace

extern "C" int qs_tree_accept_greedy(const int64_t* tokens, const int64_t* argmax, const int32_t* parents, const int32_t* cu_seqlens_q,
                                     int num_tokens, int batch, int max_accept, int32_t* accept_idx, int32_t* accept_lens, int64_t* last_row,
                                     int64_t* next_token, qs_stream_t stream) {
    QS_REQUIRE(tokens && argmax && parents && cu_seqlens_q && accept_idx && accept_lens, "tree_accept_greedy: null pointer");
    QS_REQUIRE(num_tokens >= 0 && batch >= 0, "tree_accept_greedy: bad sizes (num_tokens=%d, batch=%d)", num_tokens, batch);
    QS_REQUIRE(max_accept >= 1 && max_accept <= MAX_PATH, "tree_accept_greedy: max_accept=%d, a path has 1 .. %d nodes", max_accept, MAX_PATH);
    QS_REQUIRE(aligned8(tokens) && aligned8(argmax) && aligned8(last_row) && aligned8(next_token),
               "tree_accept_greedy: tokens, argmax, last_row and next_token must be 8-byte aligned");
    if (batch == 0 || num_tokens == 0) return QS_OK;
    hipLaunchKernelGGL(tree_accept_greedy_kernel, dim3(batch), dim3(64), 0, (hipStream_t)stream, tokens, argmax, parents, cu_seqlens_q, num_tokens,
                       max_accept, accept_idx, accept_lens, last_row, next_token);
    return qs_launch_status("tree_accept_greedy");
}

extern "C" int qs_kv_cache_commit_path_layers(const int64_t* layer_tables, int num_layers, const int32_t* past_lens, const int32_t* accept_idx,
                                              const int32_t* accept_lens, int batch, int max_accept, int max_blocks, int kv_head_num,
                                              int tokens_per_block, int size_per_token, int int4_kv_cache, int kv_cache_with_zeros,
                                              qs_stream_t stream) {
    QS_REQUIRE(layer_tables && past_lens && accept_idx && accept_lens, "kv_cache_commit_path_layers: null pointer");
    QS_REQUIRE(aligned8(layer_tables), "kv_cache_commit_path_layers: layer_tables must be 8-byte aligned");
    QS_REQUIRE(num_layers >= 1 && num_layers <= 32767, "kv_cache_commit_path_layers: num_layers=%d (1 .. 32767)", num_layers);
    QS_REQUIRE(batch >= 0 && max_accept >= 0 && max_blocks > 0 && kv_head_num > 0, "kv_cache_commit_path_layers: bad sizes");
    QS_REQUIRE(max_accept <= MAX_PATH, "kv_cache_commit_path_layers: max_accept=%d, a path has at most %d nodes", max_accept, MAX_PATH);
    if (tokens_per_block != SLOTS || !kv_cache_with_zeros) {
        qs_set_error("kv_cache_commit_path_layers: only tokens_per_block=64 and zero-point KV caches are supported");
        return QS_ENOSUP;
    }
    const int dhb = int4_kv_cache ? 64 : 128;            // bytes per cached token and head (head_dim 128)
    QS_REQUIRE(size_per_token == kv_head_num * dhb, "kv_cache_commit_path_layers: size_per_token=%d, expected %d", size_per_token,
               kv_head_num * dhb);
    if (batch == 0 || max_accept == 0) return QS_OK;
    const dim3 grid(kv_head_num, 2 * num_layers, batch), block(256);
    if (int4_kv_cache)
        hipLaunchKernelGGL(kv_commit_path_layers_kernel<64>, grid, block, 0, (hipStream_t)stream, layer_tables, past_lens, accept_idx, accept_lens,
                           max_accept, max_blocks, kv_head_num);
    else
        hipLaunchKernelGGL(kv_commit_path_layers_kernel<128>, grid, block, 0, (hipStream_t)stream, layer_tables, past_lens, accept_idx, accept_lens,
                           max_accept, max_blocks, kv_head_num);
    return qs_launch_status("kv_cache_commit_path_layers");
}
