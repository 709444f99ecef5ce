// append_window.hip -- append attention under a SLIDING WINDOW for MI355X (gfx950): qs_append_attention's rows, layout and de-quantised
// values with the rule "the key at position j is visible to the query at position p iff p - W < j <= p" (transformers'
// kv_idx > q_idx - sliding_window; the token itself counts), W >= 1.  Row t of sequence b sits at p = past + t: it sees the cached keys
// [max(0, p - W + 1), past) and the new keys [max(past, p - W + 1), p].  K / V are written for every token exactly as without a window
// (qs_append_rope_update_kv_cache is the writer of both).
//
// The walk is append_walk.h's walk_keys with its third policy, SlidingWindow; this file chooses where it begins:
//   * a query tile of tq tokens from t0 on starts at page max(0, past + t0 - W + 1) / 64 - the first page its FIRST row can see; the
//     pages below are never requested, so the chain is bounded by (W + tq) / 64 + 2 pages whatever the past - and at the tile of new
//     keys max(0, t0 - W + 1) / 64 (n > W: the early chunks of a long prompt pass fall out of the late rows' windows);
//   * pages and tiles whose first key lies above the lower edge of the wave's last row, past + t_last - W, are inside every row's
//     window and take the existing unmasked path; the edge tiles in between - at most ceil(tq / 64) + 1 pages - get the lower mask
//     next to the masks the walk already has (the end of the past, the causal diagonal);
//   * the first tiles can be fully masked for the later rows of the tile: the guarded rescale of softmax_tile_masked carries a row
//     whose maximum is still -inf (append_walk.h says how).  Every row sees at least itself, so no row ends empty.
// Un-split only: the window bounds the chain and the grid is the un-split one, batch * Hkv * q_tiles workgroups.  Split-KV, the tree
// mask and shared prefixes under a window are not built, and nothing is silently un-windowed: those entries take no window, and the
// Python layer refuses the combination with the reason.  window = 0 is "no window" (qs_append_attention's launch); window < 0 is
// QS_EINVAL before any device call.
#include "append_walk.h"

namespace {

using namespace qs_flash;
using namespace qs_append;

template <bool INT4>
__global__ __launch_bounds__(64 * NWV, 2) void append_window_kernel(const _Float16* __restrict__ qkv, _Float16* __restrict__ out,
                                                                   const int* __restrict__ cu_q, const int* __restrict__ past_lens,
                                                                   const int64_t* __restrict__ kv_pointers, int num_heads, int num_kv_heads,
                                                                   int max_blocks, int tq, int64_t qkv_stride0, int64_t o_stride0, int window,
                                                                   float scale_log2) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // grid = (KV heads, query tiles, sequences); the query tiles of a sequence run last-to-first, as in append_attention.hip
    const int hkv = blockIdx.x, qt = (int)(gridDim.y - 1 - blockIdx.y), b = blockIdx.z;
    const int G = num_heads / num_kv_heads;
    const int q_start = cu_q[b], n = cu_q[b + 1] - q_start;
    const int tok0 = qt * tq;
    if (tok0 >= n) return;
    const int past = clamp_past(past_lens[b], max_blocks);
    const int W = window < past + n ? window : past + n;          // (a longer window never binds; keeps the sums below in int range)
    const int first = past + tok0 - W + 1 > 0 ? past + tok0 - W + 1 : 0;     // the first key the tile's first row sees
    const int np_all = (past + BN - 1) / BN;
    const int p0 = first < past ? first / BN : np_all;            // first >= past: no cached key is visible, no page is walked
    const int new0 = tok0 - W + 1 > 0 ? (tok0 - W + 1) / BN : 0;
    const SlidingWindow win = {past - W, p0 * BN, past, new0};
    const int64_t* ktab = kv_pointers + (size_t)b * 2 * max_blocks;

    v16f oacc[4];
    float m_run, l_run;
    if (!walk_keys<INT4>(smem, qkv, ktab + p0, ktab + max_blocks + p0, num_heads, num_kv_heads, hkv, G, q_start, n, tok0, tq, np_all - p0,
                         past - p0 * BN, true, qkv_stride0, scale_log2, CausalNewKeys(), lane, wave, oacc, m_run, l_run, win))
        return;                                          // (behind the last barrier)
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    const float inv = l_tot > 0.f ? 1.0f / l_tot : 0.f;
    store_normalised_rows(smem, wave, oacc, inv, out, q_start, n, tok0, tq, G, hkv, o_stride0);
}

}  // namespace

extern "C" int qs_append_attention_window(const void* qkv, void* out, const int32_t* cu_seqlens_q, const int32_t* past_lens,
                                          const int64_t* kv_pointers, int num_tokens, int batch, int max_seqlen_q, int max_blocks,
                                          int num_heads, int num_kv_heads, int head_dim, int64_t qkv_stride0, int64_t out_stride0,
                                          int tokens_per_block, int size_per_token, int int4_kv_cache, int kv_cache_with_zeros, int window,
                                          qs_stream_t stream) {
    QS_REQUIRE(window >= 0, "append_attention_window: window=%d (0 = no window, >= 1 = a row sees that many keys, itself included)", window);
    AppendArgs a;
    if (const int bad = check_append_args(qkv, out, cu_seqlens_q, past_lens, kv_pointers, num_tokens, batch, max_seqlen_q, max_blocks, num_heads,
                                          num_kv_heads, head_dim, qkv_stride0, out_stride0, tokens_per_block, size_per_token, int4_kv_cache,
                                          kv_cache_with_zeros, stream, &a); bad != QS_OK)
        return bad;
    int plan3[3];
    const int rc = qs_append_attention_plan(batch, max_seqlen_q, num_heads, num_kv_heads, plan3);
    if (rc != QS_OK || a.empty()) return rc;
    const AppendPlan p = {plan3[0], plan3[1], plan3[2]};
    if (window == 0) return qs_append_launch(a, p);
    return launch_kernel_pair<append_window_kernel<true>, append_window_kernel<false>>(
        "append_attention_window", "append_attention_window", a.int4, dim3(a.num_kv_heads, p.q_tiles, a.batch), dim3(64 * p.waves), a.stream,
        a.qkv, a.out, a.cu_seqlens_q, a.past_lens, a.kv_pointers, a.num_heads, a.num_kv_heads, a.max_blocks, p.tile_tokens, a.qkv_stride0,
        a.out_stride0, window);
}
