// append_attention.hip -- append attention for MI355X (gfx950): n >= 1 new tokens of a sequence attend to the `past` tokens that
// already sit in its quantised KV4 / KV8 pages and, causally, to one another (fp16, head_dim 128, GQA).
//
// No reference counterpart (the reference has prefill over fp16 k/v and single-token decode only).  Semantics:
// query row i of sequence b sees keys 0 .. past + i;  keys < past are DE-QUANTISED FROM THE PAGES with the values of the decode
// kernels (KV4: exact nibble -> fp16, one fp16 fma with half(scale), half(-scale * zero);  KV8: fp32 scale * (u8 - zero), rounded
// to fp16), keys >= past are the rotated k / raw v of this call, read in fp16 from the packed qkv buffer.  fp32 softmax, scale
// 1/sqrt(128), fp16 output.  past = 0 is the prefill attention, n = 1 the decode attention.
//
// Mapping: the key loop is the prefill provider's, by construction - both kernels are built on the tile core of flash_tile.h (swapped
// products S^T = K Q^T / O^T = V^T P^T on v_mfma_f32_32x32x16_f16, 64-key tiles in LDS - K with a 16-byte XOR swizzle, V transposed on
// read by ds_read_b64_tr_b16 -, lazy running maximum, O out through LDS as whole rows); what differs from flash_prefill.hip is WHO the
// 128 rows of a workgroup are and WHERE a tile comes from:
//   * workgroup = (sequence, KV head, query tile); its rows are (token, head-in-group) pairs, row r = G * token + g, so the G query
//     heads of a KV group share every staged tile: a cached byte is fetched once per (sequence, KV head, query tile) - the decode
//     kernels' rule, because with a long `past` and a short n this op is bound by the cache bytes as decode is.  The causal limit
//     of a row is that of its token;
//   * phase 1, tiles 0 .. ceil(past / 64) - 1 = the pages: while tile t is computed the LDS-DMA drops this head's raw slice of page
//     t + 1 (4 KiB K + 4 KiB V for KV4, scales and zeros) into the OTHER tile buffers, each wave its 16 tokens into the rows they
//     will occupy; behind the P.V products thread (token, quarter) reads its 16 (KV4) / 32 (KV8) bytes back, de-quantises them and
//     writes four 16-byte fp16 chunks of K and of V over them - the image the MFMA loop reads is the same as for fp16 tiles, no
//     staging registers, no LDS beyond the two tile buffers.  Slots >= past of the last page are written as zeros (they may hold
//     anything, NaN scales included) and masked;
//   * phase 2, the new tokens' fp16 k / v rows from qkv by LDS-DMA in 64-key tiles with the causal mask, exactly as in the prefill
//     provider.
// One barrier per tile, two LDS buffers, online softmax across both phases.  No split-KV: a workgroup walks the whole past.
// The walk itself (both phases, the staging and the key loop) is append_walk.h's walk_keys, shared with the split-KV and the tree
// kernels; this file chooses the rows and the key range and stores the normalised result.
#include "append_walk.h"

namespace {

using namespace qs_flash;
using namespace qs_append;      // the walk and the leaves shared with the split-KV and the tree kernels (append_walk.h)

template <bool INT4>
__global__ __launch_bounds__(64 * NWV, 2) void append_attention_kernel(const _Float16* __restrict__ qkv, _Float16* __restrict__ out,
                                                                      const int* __restrict__ cu_q, const int* __restrict__ past_lens,
                                                                      const int64_t* __restrict__ kv_pointers, int num_heads,
                                                                      int num_kv_heads, int max_blocks, int tq, int64_t qkv_stride0,
                                                                      int64_t o_stride0, float scale_log2) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // grid = (KV heads, query tiles, sequences); the query tiles of a sequence run last-to-first (the ones with the most keys first)
    const int hkv = blockIdx.x, qt = (int)(gridDim.y - 1 - blockIdx.y), b = blockIdx.z;
    const int G = num_heads / num_kv_heads;
    const int q_start = cu_q[b], n = cu_q[b + 1] - q_start;
    const int tok0 = qt * tq;                            // first new token of this tile
    if (tok0 >= n) return;                               // (n = 0: nothing read, nothing written)
    const int past = clamp_past(past_lens[b], max_blocks);
    const int np = (past + BN - 1) / BN;                 // phase 1: every page of the sequence
    const int64_t* ktab = kv_pointers + (size_t)b * 2 * max_blocks;

    v16f oacc[4];
    float m_run, l_run;
    if (!walk_keys<INT4>(smem, qkv, ktab, ktab + max_blocks, num_heads, num_kv_heads, hkv, G, q_start, n, tok0, tq, np, past, true, qkv_stride0,
                         scale_log2, CausalNewKeys(), lane, wave, oacc, m_run, l_run))
        return;                                          // (behind the last barrier)
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    const float inv = l_tot > 0.f ? 1.0f / l_tot : 0.f;       // a row that saw no key: exactly 0
    store_normalised_rows(smem, wave, oacc, inv, out, q_start, n, tok0, tq, G, hkv, o_stride0);
}

}  // namespace

extern "C" int qs_append_attention_plan(int batch, int max_seqlen_q, int num_heads, int num_kv_heads, int* plan3) {
    QS_REQUIRE(plan3, "append attention plan: null output");
    plan3[0] = plan3[1] = plan3[2] = 0;
    QS_REQUIRE(batch >= 0 && max_seqlen_q >= 0, "append_attention: negative batch / max_seqlen_q");
    QS_REQUIRE(num_heads > 0 && num_kv_heads > 0 && num_heads % num_kv_heads == 0,
               "append_attention: bad head counts H=%d Hkv=%d", num_heads, num_kv_heads);
    if (num_heads / num_kv_heads > MAX_G) {
        qs_set_error("append_attention: num_heads/num_kv_heads = %d not in 1..%d", num_heads / num_kv_heads, MAX_G);
        return QS_ENOSUP;
    }
    if (batch == 0 || max_seqlen_q == 0) return QS_OK;
    const AppendPlan p = attn_plan::plan_append(max_seqlen_q, num_heads, num_kv_heads);
    plan3[0] = p.tile_tokens, plan3[1] = p.q_tiles, plan3[2] = p.waves;
    return QS_OK;
}

int qs_append_launch(const AppendArgs& a, const AppendPlan& p) {
    return launch_kernel_pair<append_attention_kernel<true>, append_attention_kernel<false>>(
        "append_attention", "append_attention", a.int4, dim3(a.num_kv_heads, p.q_tiles, a.batch), dim3(64 * p.waves), a.stream, a.qkv, a.out,
        a.cu_seqlens_q, a.past_lens, a.kv_pointers, a.num_heads, a.num_kv_heads, a.max_blocks, p.tile_tokens, a.qkv_stride0, a.out_stride0);
}

extern "C" int qs_append_attention(const void* qkv, void* out, const int32_t* cu_seqlens_q, const int32_t* past_lens,
                                   const int64_t* kv_pointers, int num_tokens, int batch, int max_seqlen_q, int max_blocks,
                                   int num_heads, int num_kv_heads, int head_dim, int64_t qkv_stride0, int64_t out_stride0,
                                   int tokens_per_block, int size_per_token, int int4_kv_cache, int kv_cache_with_zeros,
                                   qs_stream_t stream) {
    AppendArgs a;
    if (const int bad = check_append_args(qkv, out, cu_seqlens_q, past_lens, kv_pointers, num_tokens, batch, max_seqlen_q, max_blocks, num_heads,
                                          num_kv_heads, head_dim, qkv_stride0, out_stride0, tokens_per_block, size_per_token, int4_kv_cache,
                                          kv_cache_with_zeros, stream, &a); bad != QS_OK)
        return bad;
    int plan3[3];
    const int rc = qs_append_attention_plan(batch, max_seqlen_q, num_heads, num_kv_heads, plan3);
    if (rc != QS_OK || a.empty()) return rc;
    return qs_append_launch(a, {plan3[0], plan3[1], plan3[2]});
}
