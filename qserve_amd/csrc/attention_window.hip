// attention_window.hip -- decode attention under a SLIDING WINDOW on the matrix cores (gfx950): the new token at position p sees key j
// iff p - W < j <= p (transformers' kv_idx > q_idx - sliding_window; the token itself counts), W >= 1 (Mistral-7B-v0.1: W = 4 096).
// The contract is qs_single_query_attention_long's - rotate q and the new k, quantise the new token's k / v into its page slot
// (kv_quant.h: the same bits, every token is written exactly as without a window), attend - over the cached tokens
// [max(0, len - W), len - 1) of len = lengths[b] plus the new one.  KV4 and KV8, G = H / Hkv in 1 .. 8, tables of any length.
//
// Mapping
//   * workgroup = (KV head, sequence, range), grid (Hkv, batch, S); S is the host's (attn_plan.h plan_decode_window: from the table's
//     length and W alone, so a captured graph keeps its grid while the lengths grow and the window moves).  The ranges are cut here, on
//     the device, from the WINDOW's pages [lo / 64, ceil((len - 1) / 64)), lo = max(0, len - W), not from the text's: npages of them
//     go evenly to nr = clamp(npages / min_pages, 1, S) ranges, and a workgroup with z >= nr leaves the empty record.  A chain is at
//     most W / 64 + 2 pages whatever the text's length: a 131 072-token text under W = 4 096 walks 64 or 65 pages per head, not 2 048.
//     A sequence shorter than W has lo = 0 and is cut exactly as attention_long.hip cuts it.
//   * the mask has ONE place.  Pages behind the first lie wholly at or above lo, and the upper end is the long kernel's `valid` (only
//     the last page is partial), so only the first page of the first range can hold a token below the window: there the walk
//     compares the token index with the per-sequence scalar lo - 64 (lo / 64) - one wave-uniform test per page (p == first page), the
//     selects behind it on that page alone, nothing on the others.
//   * a range that is ENTIRELY masked cannot exist with this cut.  For W >= 2 and len >= 2, lo <= len - 2: token lo is cached, visible
//     and sits in page lo / 64, the first page of the first range, so that page keeps at least one key; every other page holds only
//     tokens >= lo; and a range has at least one page unless npages = 0.  The running maximum of every wave that walks a page is
//     therefore a real score, and the softmax needs no guard the long kernel does not have.  W = 1 (lo = len - 1: no cached token is
//     visible) and len = 1 walk NO cached page at all - npages is set to 0, not to the one page that would be fully masked -: range 0
//     is the writer and the result is the new token's own term, as past = 0 is today.
//   * everything else - range nr - 1 writes and adds the new token, 4 waves own whole pages begin + w, begin + w + 4, ..., pages travel
//     HBM -> LDS by LDS-DMA into wave-private rings of 2 stages, page addresses are staged 256 at a time, de-quantisation is
//     append_dequant.h's dequant8 between ds_read and the MFMA operand, records have attn_plan::decode_split_bytes' layout and
//     qs_launch_attention_merge joins them in range order (no cross-workgroup wait inside the launch, results bit-identical run to run
//     and under graph replay) - is attention_long_body.h, the statements of attention_long.hip's kernels; that file's header has
//     the reasons.
// LDS: the long kernel's budget, 78 KiB (KV4: two workgroups per CU) / 142 KiB (KV8: one) of 160; the window adds a scalar, no LDS.
// Not built: ring-buffer tables, giving pages that fell out of the window back to the pool, attention sinks.
// Refused (QS_EINVAL, before any device call): window < 0.  window = 0 is "no window": qs_single_query_attention_long's result.
#include "attention_long_walk.h"

namespace {

using namespace qs_long;

template <bool INT4>
__global__ __launch_bounds__(TPB) void decode_window_kernel(
    const _Float16* __restrict__ q, const _Float16* __restrict__ k, const _Float16* __restrict__ v,
    const int64_t* __restrict__ kv_pointers, const int* __restrict__ lengths, _Float16* __restrict__ out, int num_heads,
    int num_kv_heads, int G, int64_t q_stride0, int64_t kv_stride0, int max_blocks, int timestep, float rope_base,
    const float2* __restrict__ rope_tab, int rope_tab_len, int S, int min_pages, float* __restrict__ ws, int window) {
    constexpr bool WINDOW = true;
#include "attention_long_body.h"
}

constexpr int NO_WINDOW = 0x7fffffff;      // window = 0 on the device: lo = max(0, len - NO_WINDOW) = 0 for every int32 length

}  // namespace

extern "C" int qs_single_query_attention_window(const void* q, const void* k, const void* v, const int64_t* kv_pointers,
                                                const int32_t* length_per_sample, void* out, int batch, int num_heads, int num_kv_heads,
                                                int head_dim, int64_t q_stride0, int64_t kv_stride0, int max_blocks, int memory_max_seqlen,
                                                int tokens_per_block, int size_per_token, int timestep, int rotary_embedding_dim,
                                                float rotary_base, int neox_rotary_style, int int4_kv_cache, int kv_cache_with_zeros,
                                                int window, int num_splits, qs_stream_t stream) {
    (void)neox_rotary_style;       // accepted, no effect: as in qs_single_query_attention
    const char* what = "single_query_attention_window";
    QS_REQUIRE(window >= 0, "%s: window=%d (0 = no window, >= 1 = the new token sees that many keys, itself included)", what, window);
    DecodeLongArgs a;
    if (const int bad = check_decode_long_args(what, q, k, v, kv_pointers, length_per_sample, out, batch, num_heads, num_kv_heads, head_dim,
                                               q_stride0, kv_stride0, max_blocks, memory_max_seqlen, tokens_per_block, size_per_token, timestep,
                                               rotary_embedding_dim, rotary_base, int4_kv_cache, kv_cache_with_zeros, num_splits, stream, &a);
        bad != QS_OK)
        return bad;
    if (batch == 0) return QS_OK;
    LongPlan plan = attn_plan::plan_decode_window(batch, num_kv_heads, a.d.G, max_blocks, window, a.int4, qs_split_workspace_capacity());
    if (num_splits >= 1) plan.splits = num_splits > attn_plan::MAX_SPLITS ? attn_plan::MAX_SPLITS : num_splits;
    return launch_long_kernels<decode_window_kernel<true>, decode_window_kernel<false>>(what, a, plan, window > 0 ? window : NO_WINDOW);
}

extern "C" int qs_single_query_attention_window_plan(int batch, int num_heads, int num_kv_heads, int max_blocks, int window,
                                                     int int4_kv_cache, int* plan3) {
    const char* what = "single_query_attention_window";
    QS_REQUIRE(plan3, "%s plan: null output", what);
    plan3[0] = plan3[1] = plan3[2] = 0;
    QS_REQUIRE(window >= 0, "%s: window=%d (0 = no window, >= 1 = the new token sees that many keys, itself included)", what, window);
    QS_REQUIRE(batch >= 0 && num_heads > 0 && num_kv_heads > 0 && num_heads % num_kv_heads == 0, "%s: bad head counts H=%d Hkv=%d", what,
               num_heads, num_kv_heads);
    QS_REQUIRE(max_blocks > 0, "%s: bad max_blocks / memory_max_seqlen", what);
    if (num_heads / num_kv_heads > 8) {
        qs_set_error("%s: num_heads/num_kv_heads = %d not in 1..8", what, num_heads / num_kv_heads);
        return QS_ENOSUP;
    }
    if (batch == 0) return QS_OK;
    const LongPlan p = attn_plan::plan_decode_window(batch, num_kv_heads, num_heads / num_kv_heads, max_blocks, window, int4_kv_cache != 0,
                                                     qs_split_workspace_capacity());
    plan3[0] = p.splits, plan3[1] = p.waves, plan3[2] = p.min_pages;
    return QS_OK;
}
