// append_tree.hip -- verification of a DRAFT TREE for MI355X (gfx950): append attention (append_attention.hip, append_attention_split.hip)
// where the n <= 64 new tokens of a sequence are the nodes of a tree in topological order - several candidates per position, as Medusa,
// EAGLE and SpecInfer draft them - and a node attends to the cached context and, among the new tokens, to ITS ANCESTORS ONLY; and the
// mover that afterwards turns the accepted root-to-leaf path into an ordinary cache.  DESIGN.md 10 ("Tree verification").
//
//   tree_mask  uint64 [T], one word per row of the packed qkv buffer: bit j of node i's word = "node i sees new token j of its own
//              sequence"; bits >= n are ignored.  The kernels assume nothing else (no j <= i, no closure): the word is the whole truth
//              among the new tokens.  The writer (attention.hip) derives a node's position from the same word - depth = popcount - 1.
//
// The attention kernels are append_walk.h's walk with another NEWKEYS policy - same rows (row r = G * token + g), same page staging,
// in-place de-quantisation, key loop and epilogues as the linear kernels; with n <= 64 there is ONE tile of new keys, every wave with a
// row computes it, and it is always masked: the row's word is loaded inside that tile's (unlikely) mask block - not before the page
// loop, where it would be two more registers carried through it -, shifted by the lane half (word >> 4 hi: the 32 key indices of a lane
// stay immediates, flash_tile.h) and tested bit by bit.  A page's prefix mask (slots >= past) goes through the same block as the word
// (2 << limit) - 1: one block of selects per tile body, and the values a chain tree masks are the linear kernels' - with chain words
// (2 << i) - 1 the results are bit-identical to qs_append_attention / qs_append_attention_split.
//   append_tree_attention_kernel<INT4>        un-split: a workgroup walks the whole past, normalised fp16 rows
//   append_tree_attention_split_kernel<INT4>  a page range per workgroup, the new keys behind the last range, partial records; merged by
//                                             append_attention_split.hip's merge kernel (mask-agnostic, reused as it is)
//
//   kv_commit_path_kernel<DHB>  after acceptance: slot past + k of every (KV head, K | V) receives the bytes - data, fp16 scale, fp16 zero -
//              of slot past + accept_idx[k], k < accept_len.  accept_idx rows increase strictly, so a source may be an earlier move's
//              destination, never a later one's - but moves run in parallel: one workgroup owns a (sequence, KV head, K | V), reads
//              EVERY source into LDS, takes a barrier, then stores.  Identity moves are skipped; nothing else in a page is written;
//              slots >= past + accept_len keep what they hold (every reader masks them).  Vector stores only.
#include "append_walk.h"
#include "kv_commit.h"

namespace {

using namespace qs_flash;
using namespace qs_append;

constexpr int MAX_TREE = BN;      // nodes per sequence: one tile of new keys, one 64-bit word per row

// The ancestor rule: row of node tok sees new key j iff j < n and bit j of words[tok].
struct TreeNewKeys {
    const uint64_t* words;        // the sequence's words (tree_mask + its first row): wave-uniform
    __device__ __forceinline__ int count(int n, int tok0, int tq) const { return n < MAX_TREE ? n : MAX_TREE; }   // any key, any row
    __device__ __forceinline__ int tiles(int tok_last, int nn) const { return nn; }
    __device__ __forceinline__ bool needs_mask(int j0, int tok_first, int n) const { return true; }
    __device__ __forceinline__ void mask(v16f (&sacc)[NKB], int hi, bool page, int page_limit, int j0, int tok_ld, int n) const {
        uint64_t w;
        if (page) {               // keys 0 .. page_limit (a masked page has page_limit < 63; below 0: no key)
            w = page_limit >= 63 ? ~0ull : page_limit < 0 ? 0ull : (2ull << page_limit) - 1;
        } else {
            w = words[tok_ld];
            if (n < MAX_TREE) w &= (1ull << n) - 1;
        }
        mask_keys_by_word(sacc, w, hi);
    }
};

template <bool INT4>
__global__ __launch_bounds__(64 * NWV, 2) void append_tree_attention_kernel(const _Float16* __restrict__ qkv, _Float16* __restrict__ out,
                                                                           const int* __restrict__ cu_q, const int* __restrict__ past_lens,
                                                                           const int64_t* __restrict__ kv_pointers,
                                                                           const uint64_t* __restrict__ tree_mask, int num_heads,
                                                                           int num_kv_heads, int max_blocks, int tq, int64_t qkv_stride0,
                                                                           int64_t o_stride0, float scale_log2) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // grid = (KV heads, query tiles, sequences), as append_attention_kernel
    const int hkv = blockIdx.x, qt = (int)(gridDim.y - 1 - blockIdx.y), b = blockIdx.z;
    const int G = num_heads / num_kv_heads;
    const int q_start = cu_q[b], n = cu_q[b + 1] - q_start;
    const int tok0 = qt * tq;
    if (tok0 >= n) return;
    const int past = clamp_past(past_lens[b], max_blocks);
    const int np = (past + BN - 1) / BN;
    const int64_t* ktab = kv_pointers + (size_t)b * 2 * max_blocks;

    v16f oacc[4];
    float m_run, l_run;
    if (!walk_keys<INT4>(smem, qkv, ktab, ktab + max_blocks, num_heads, num_kv_heads, hkv, G, q_start, n, tok0, tq, np, past, true, qkv_stride0,
                         scale_log2, TreeNewKeys{tree_mask + q_start}, lane, wave, oacc, m_run, l_run))
        return;
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    const float inv = l_tot > 0.f ? 1.0f / l_tot : 0.f;       // a row that sees no key (past 0, empty word): exactly 0
    store_normalised_rows(smem, wave, oacc, inv, out, q_start, n, tok0, tq, G, hkv, o_stride0);
}

template <bool INT4>
__global__ __launch_bounds__(64 * NWV, 2) void append_tree_attention_split_kernel(const _Float16* __restrict__ qkv, float* __restrict__ ws,
                                                                                 const int* __restrict__ cu_q, const int* __restrict__ past_lens,
                                                                                 const int64_t* __restrict__ kv_pointers,
                                                                                 const uint64_t* __restrict__ tree_mask, int num_heads,
                                                                                 int num_kv_heads, int max_blocks, int tq, int q_tiles,
                                                                                 int splits, int64_t qkv_stride0, float scale_log2) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // grid = (KV heads, query tiles x splits, sequences), ranges, EMPTY rule and records: append_attention_split_kernel's
    const int hkv = blockIdx.x, b = blockIdx.z;
    const int split = (int)blockIdx.y % splits, qt = q_tiles - 1 - (int)blockIdx.y / splits;
    const int G = num_heads / num_kv_heads;
    const int q_start = cu_q[b], n = cu_q[b + 1] - q_start;
    const int tok0 = qt * tq;
    if (tok0 >= n) return;
    const int past_all = clamp_past(past_lens[b], max_blocks);
    const PageRange pr = split_range(past_all, split, splits);
    const bool with_new = split == splits - 1;
    if (pr.np == 0 && !with_new) return;
    const int64_t* ktab = kv_pointers + (size_t)b * 2 * max_blocks + pr.p0;

    v16f oacc[4];
    float m_run, l_run;
    if (!walk_keys<INT4>(smem, qkv, ktab, ktab + max_blocks, num_heads, num_kv_heads, hkv, G, q_start, n, tok0, tq, pr.np, past_all - pr.p0 * BN,
                         with_new, qkv_stride0, scale_log2, TreeNewKeys{tree_mask + q_start}, lane, wave, oacc, m_run, l_run))
        return;
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    const size_t wg = ((size_t)b * q_tiles + qt) * num_kv_heads + hkv;
    store_partial_record(ws + ((wg * splits + split) * NWV + wave) * REC_FLOATS, oacc, m_run, l_tot);
}

// ---- path commit.  grid = (KV heads, 2 = K | V, sequences), 256 threads; DHB = bytes per cached token and head (64 KV4, 128 KV8).
// A page: data [Hkv][64][DHB], then fp16 scales [Hkv][64], then fp16 zeros [Hkv][64].  Move k: thread (k, c) of the data pass copies
// the 16-byte chunk c of the token, thread k of the parameter pass its scale and zero.  A move whose source or destination lies beyond
// the pointer table, or whose index is not in 0 .. 63, is dropped.  The moves themselves are kv_commit.h's, shared with the all-layers
// launch of tree_accept.hip.
template <int DHB>
__global__ __launch_bounds__(256) void kv_commit_path_kernel(const int64_t* __restrict__ kv_pointers, const int* __restrict__ past_lens,
                                                             const int* __restrict__ accept_idx, const int* __restrict__ accept_lens,
                                                             int max_accept, int max_blocks, int kv_head_num) {
    constexpr int CH = DHB / 16;                         // 16-byte chunks per token
    __shared__ v4u s_data[MAX_TREE * CH];
    __shared__ u32 s_par[MAX_TREE];                      // (scale, zero) as two fp16
    const int hkv = blockIdx.x, which = blockIdx.y, b = blockIdx.z;
    int m = accept_lens[b];
    m = m < 0 ? 0 : m > max_accept ? max_accept : m;
    const int past = past_lens[b];
    const int64_t* tab = kv_pointers + ((size_t)b * 2 + which) * max_blocks;
    const int* idx = accept_idx + (size_t)b * max_accept;
    qs_commit::commit_path_moves<DHB>(tab, idx, m, past, hkv, max_blocks, kv_head_num, s_data, s_par);      // the rule itself: kv_commit.h
}

}  // namespace

namespace {

int tree_launch(const AppendArgs& a, const AppendPlan& p) {
    return launch_kernel_pair<append_tree_attention_kernel<true>, append_tree_attention_kernel<false>>(
        "append_tree_attention", "append_tree_attention", a.int4, dim3(a.num_kv_heads, p.q_tiles, a.batch), dim3(64 * p.waves), a.stream, a.qkv,
        a.out, a.cu_seqlens_q, a.past_lens, a.kv_pointers, a.tree_mask, a.num_heads, a.num_kv_heads, a.max_blocks, p.tile_tokens, a.qkv_stride0,
        a.out_stride0);
}

int tree_split_launch(const AppendArgs& a, const AppendPlan& p, int wanted_splits) {
    float* ws = nullptr;
    const int splits = qs_append_split_resolve(wanted_splits, a, p, &ws);
    if (!ws) return tree_launch(a, p);           // one split, or no workspace (first use inside a capture): the un-split launch
    const int lrc = launch_kernel_pair<append_tree_attention_split_kernel<true>, append_tree_attention_split_kernel<false>>(
        "append_tree_attention", "append_tree_attention_split", a.int4, dim3(a.num_kv_heads, p.q_tiles * splits, a.batch), dim3(64 * p.waves),
        a.stream, a.qkv, ws, a.cu_seqlens_q, a.past_lens, a.kv_pointers, a.tree_mask, a.num_heads, a.num_kv_heads, a.max_blocks, p.tile_tokens,
        p.q_tiles, splits, a.qkv_stride0);
    return lrc != QS_OK ? lrc : qs_append_merge_launch(ws, a, p, splits);
}

}  // namespace

extern "C" int qs_append_tree_attention(const void* qkv, void* out, const int32_t* cu_seqlens_q, const int32_t* past_lens,
                                        const int64_t* kv_pointers, const uint64_t* tree_mask, int num_tokens, int batch, int max_seqlen_q,
                                        int max_blocks, int num_heads, int num_kv_heads, int head_dim, int64_t qkv_stride0,
                                        int64_t out_stride0, int tokens_per_block, int size_per_token, int int4_kv_cache,
                                        int kv_cache_with_zeros, int max_past, int num_splits, qs_stream_t stream) {
    AppendArgs a;
    if (const int bad = check_append_args(qkv, out, cu_seqlens_q, past_lens, kv_pointers, num_tokens, batch, max_seqlen_q, max_blocks, num_heads,
                                          num_kv_heads, head_dim, qkv_stride0, out_stride0, tokens_per_block, size_per_token, int4_kv_cache,
                                          kv_cache_with_zeros, stream, &a); bad != QS_OK)
        return bad;
    QS_REQUIRE(tree_mask, "append_tree_attention: null tree_mask");
    QS_REQUIRE((reinterpret_cast<uintptr_t>(tree_mask) & 7) == 0, "append_tree_attention: tree_mask must be 8-byte aligned");
    QS_REQUIRE(max_seqlen_q <= MAX_TREE, "append_tree_attention: max_seqlen_q=%d, a tree has at most %d nodes per sequence", max_seqlen_q,
               MAX_TREE);
    QS_REQUIRE(num_splits >= 0, "append_tree_attention: num_splits=%d (0 = ask the planner, >= 1 = forced)", num_splits);
    a.tree_mask = tree_mask;
    int plan5[5];
    const int rc = qs_append_attention_split_plan(batch, max_seqlen_q, table_hint(max_past, max_blocks), num_heads, num_kv_heads, int4_kv_cache, plan5);
    if (rc != QS_OK || a.empty()) return rc;
    return tree_split_launch(a, {plan5[0], plan5[1], plan5[2]}, num_splits > 0 ? num_splits : plan5[3]);
}

extern "C" int qs_kv_cache_commit_path(const int64_t* kv_pointers, const int32_t* past_lens, const int32_t* accept_idx,
                                       const int32_t* accept_lens, int batch, int max_accept, int max_blocks, int kv_head_num,
                                       int tokens_per_block, int size_per_token, int int4_kv_cache, int kv_cache_with_zeros,
                                       qs_stream_t stream) {
    QS_REQUIRE(kv_pointers && past_lens && accept_idx && accept_lens, "kv_cache_commit_path: null pointer");
    QS_REQUIRE(batch >= 0 && max_accept >= 0 && max_blocks > 0 && kv_head_num > 0, "kv_cache_commit_path: bad sizes");
    QS_REQUIRE(max_accept <= MAX_TREE, "kv_cache_commit_path: max_accept=%d, a path has at most %d nodes", max_accept, MAX_TREE);
    if (tokens_per_block != BN || !kv_cache_with_zeros) {
        qs_set_error("kv_cache_commit_path: only tokens_per_block=64 and zero-point KV caches are supported");
        return QS_ENOSUP;
    }
    const int dhb = int4_kv_cache ? DH / 2 : DH;
    QS_REQUIRE(size_per_token == kv_head_num * dhb, "kv_cache_commit_path: size_per_token=%d, expected %d", size_per_token, kv_head_num * dhb);
    if (batch == 0 || max_accept == 0) return QS_OK;
    const dim3 grid(kv_head_num, 2, batch), block(256);
    if (int4_kv_cache)
        hipLaunchKernelGGL(kv_commit_path_kernel<DH / 2>, grid, block, 0, (hipStream_t)stream, kv_pointers, past_lens, accept_idx, accept_lens,
                           max_accept, max_blocks, kv_head_num);
    else
        hipLaunchKernelGGL(kv_commit_path_kernel<DH>, grid, block, 0, (hipStream_t)stream, kv_pointers, past_lens, accept_idx, accept_lens,
                           max_accept, max_blocks, kv_head_num);
    return qs_launch_status("kv_cache_commit_path");
}
