// append_attention_split.hip -- split-KV append attention for MI355X (gfx950): the op of append_attention.hip (n new tokens of a
// sequence over its quantised KV4 / KV8 pages and, causally, over one another) for LONG contexts at SMALL batch, where the un-split
// launch - one workgroup per (sequence, KV head, query tile) that walks the whole past - leaves most of the 256 CUs idle behind a few
// serial chains of pages (B = 1, 32 / 8 heads, past 8 192, n = 8: 8 workgroups of 128 page tiles each).  DESIGN.md 10.
//
// Two launches on one stream, no in-launch wait, no atomics (a dependent kernel boundary is the cheapest cross-workgroup
// edge on this chip):
//   1. append_attention_split_kernel<INT4>, grid (KV heads, query tiles x splits, sequences).  The key loop, the row mapping
//      (row r = G * token + g), the page staging and the in-place de-quantisation are append_attention.hip's (the tile core of
//      flash_tile.h, the leaves of append_dequant.h); what differs is the key range and the way the result leaves:
//        * split s of sequence b walks pages [s pps, min((s + 1) pps, np_b)) with np_b = ceil(past_lens[b] / 64),
//          pps = ceil(np_b / splits) - computed ON THE DEVICE from the sequence's own length, so the host's max_past is a hint
//          for the planner and nothing a result depends on;
//        * the LAST split (s = splits - 1) also runs phase 2, the new tokens' fp16 keys with the causal mask: with ceil-sized
//          ranges the last one is the shortest (often empty), so the extra tiles land where there is room for them;
//        * a split without a page and without phase 2 is EMPTY: it returns at once and writes nothing.  The merge kernel recomputes
//          the same test from past_lens and never reads an empty split's (stale) records;
//        * no normalisation: every wave with a valid row writes the partial record of its 32 rows - un-normalised fp32 O[128], the
//          running maximum m (log2 domain; the lazy one: O and l are relative to it, whatever it is) and the fp32 sum l.
//   2. append_attention_merge_kernel, grid (KV heads, query tiles x 4, sequences): per (token, head)
//        M = max_s m_s,  out = sum_s 2^(m_s - M) O_s / sum_s 2^(m_s - M) l_s   in fp32, fp16 out through out_stride0;
//      m_s = -inf gives weight 0 (no -inf - (-inf)); a row that saw no key is exactly 0, the un-split kernel's rule.
//
// Workspace record (fp32), one per (workgroup of the un-split grid, split, wave): 32 rows x 130 values = 16 640 bytes, TRANSPOSED so
// that the accumulator registers leave as they are - [32 chunks of 4 dims][32 rows][4] then m[32], l[32]: lane (row li, half hi)
// holds dims 32 d + 8 rq + 4 hi .. + 3 of its row in oacc[d][4 rq ..], i.e. chunk 8 d + 2 rq + hi; a store instruction writes
// 1 KiB of consecutive bytes per wave (16 of them per lane, no LDS round trip, no extra registers), and the merge reads the same
// 16-byte pieces back, 32 rows = 512 consecutive bytes per chunk.  Rows of a written block that hold no token carry finite
// garbage nobody reads.  The area is the library's split-KV workspace (attention_mfma.hip: 32 MiB per device and bound stream,
// allocated on the first eager use, never during a capture); without it - or with one split - the entry runs the un-split launcher.
#include "append_walk.h"

namespace {

using namespace qs_flash;
using namespace qs_append;      // REC_FLOATS, MAX_SPLITS, the walk and the record's store: append_walk.h

template <bool INT4>
__global__ __launch_bounds__(64 * NWV, 2) void append_attention_split_kernel(const _Float16* __restrict__ qkv, float* __restrict__ ws,
                                                                            const int* __restrict__ cu_q, const int* __restrict__ past_lens,
                                                                            const int64_t* __restrict__ kv_pointers, int num_heads,
                                                                            int num_kv_heads, int max_blocks, int tq, int q_tiles, int splits,
                                                                            int64_t qkv_stride0, float scale_log2) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // grid = (KV heads, query tiles x splits, sequences); the splits of a query tile are neighbours, the tiles run last-to-first
    const int hkv = blockIdx.x, b = blockIdx.z;
    const int split = (int)blockIdx.y % splits, qt = q_tiles - 1 - (int)blockIdx.y / splits;
    const int G = num_heads / num_kv_heads;
    const int q_start = cu_q[b], n = cu_q[b + 1] - q_start;
    const int tok0 = qt * tq;                            // first new token of this tile
    if (tok0 >= n) return;                               // (n = 0: nothing read, nothing written)
    const int past_all = clamp_past(past_lens[b], max_blocks);
    // this split's pages [p0, p0 + np) of the sequence's; `past` = the cached tokens counted from page p0 (beyond np * BN for every
    // range but the one that holds the last page: no slot of those ranges is masked)
    const PageRange pr = split_range(past_all, split, splits);
    const bool with_new = split == splits - 1;           // the last split also serves phase 2
    if (pr.np == 0 && !with_new) return;                 // EMPTY: no record (the merge recomputes this test)
    const int64_t* ktab = kv_pointers + (size_t)b * 2 * max_blocks + pr.p0;

    v16f oacc[4];
    float m_run, l_run;
    if (!walk_keys<INT4>(smem, qkv, ktab, ktab + max_blocks, num_heads, num_kv_heads, hkv, G, q_start, n, tok0, tq, pr.np, past_all - pr.p0 * BN,
                         with_new, qkv_stride0, scale_log2, CausalNewKeys(), lane, wave, oacc, m_run, l_run))
        return;                                          // (behind the last barrier; the merge skips this wave's block by the same test)
    // ---- epilogue: the wave's partial record, straight from the accumulator registers (layout: the head of this file)
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    const size_t wg = ((size_t)b * q_tiles + qt) * num_kv_heads + hkv;
    store_partial_record(ws + ((wg * splits + split) * NWV + wave) * REC_FLOATS, oacc, m_run, l_tot);
}

// One workgroup per (KV head, query tile, wave block of 32 rows, sequence); thread (row li = tid & 31, tid >> 5) merges the chunks
// (tid >> 5) + 8 i, i = 0 .. 3, of its row over the non-empty splits.
__global__ __launch_bounds__(256) void append_attention_merge_kernel(const float* __restrict__ ws, _Float16* __restrict__ out,
                                                                    const int* __restrict__ cu_q, const int* __restrict__ past_lens,
                                                                    int num_heads, int num_kv_heads, int max_blocks, int tq, int q_tiles,
                                                                    int splits, int64_t o_stride0) {
    const int hkv = blockIdx.x, b = blockIdx.z;
    const int qt = (int)blockIdx.y / NWV, wave = (int)blockIdx.y % NWV;
    const int G = num_heads / num_kv_heads;
    const int q_start = cu_q[b], n = cu_q[b + 1] - q_start;
    const int tok0 = qt * tq;
    if (tok0 >= n || wave * 32 >= tq * G || tok0 + (wave * 32) / G >= n) return;      // no record: the split kernel's tests
    const int li = threadIdx.x & 31, c0 = threadIdx.x >> 5;
    const int r = wave * 32 + li, tok = tok0 + r / G;
    if (r >= tq * G || tok >= n) return;                 // a row of the block without a token
    int past = past_lens[b];
    past = past < 0 ? 0 : past > max_blocks * BN ? max_blocks * BN : past;
    const int np_all = (past + BN - 1) / BN;
    const int pps = (np_all + splits - 1) / splits;
    const size_t wg = ((size_t)b * q_tiles + qt) * num_kv_heads + hkv;
    const float* const rec0 = ws + (wg * splits * NWV + wave) * REC_FLOATS;
    const size_t rec_step = (size_t)NWV * REC_FLOATS;    // from one split's block to the next
    auto written = [&](int s) { return s * pps < np_all || s == splits - 1; };

    float M = -INFINITY;
    for (int s = 0; s < splits; ++s)
        if (written(s)) M = fmaxf(M, rec0[s * rec_step + 32 * DH + li]);
    v4f acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = (v4f){0.f, 0.f, 0.f, 0.f};
    float den = 0.f;
    for (int s = 0; s < splits; ++s) {
        if (!written(s)) continue;
        const float* const rec = rec0 + s * rec_step;
        const float m = rec[32 * DH + li];
        if (m == -INFINITY) continue;                    // the split saw no key of this row: l = 0, O = 0 (and M may be -inf too)
        const float w = __builtin_amdgcn_exp2f(m - M);
        den += w * rec[32 * DH + 32 + li];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] += w * *reinterpret_cast<const v4f*>(rec + (c0 + 8 * i) * 128 + li * 4);
    }
    const float inv = den > 0.f ? 1.0f / den : 0.f;       // no key at all: exactly 0
    _Float16* const orow = out + (size_t)(q_start + tok) * o_stride0 + (size_t)(hkv * G + r % G) * DH;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const h4 o = {(_Float16)(acc[i][0] * inv), (_Float16)(acc[i][1] * inv), (_Float16)(acc[i][2] * inv), (_Float16)(acc[i][3] * inv)};
        *reinterpret_cast<h4*>(orow + (c0 + 8 * i) * 4) = o;
    }
}

}  // namespace

// What every split-KV append launcher needs besides its own kernel (attn_host.h; append_tree.hip is the other user).
int qs_append_split_resolve(int wanted, const AppendArgs& a, const AppendPlan& p, float** ws) {
    const size_t per_split = attn_plan::append_split_bytes((size_t)a.batch * a.num_kv_heads * p.q_tiles);
    const int splits = attn_plan::fit_splits(wanted, per_split, qs_split_workspace_capacity(), MAX_SPLITS);
    *ws = splits > 1 ? qs_split_workspace(per_split * splits, a.stream) : nullptr;
    return *ws ? splits : 1;
}
int qs_append_merge_launch(const float* ws, const AppendArgs& a, const AppendPlan& p, int splits) {
    hipLaunchKernelGGL(append_attention_merge_kernel, dim3(a.num_kv_heads, p.q_tiles * NWV, a.batch), dim3(256), 0, a.stream, ws, a.out,
                       a.cu_seqlens_q, a.past_lens, a.num_heads, a.num_kv_heads, a.max_blocks, p.tile_tokens, p.q_tiles, splits, a.out_stride0);
    return qs_launch_status("append_attention_merge");
}

int qs_append_split_launch(const AppendArgs& a, const AppendPlan& p, int wanted_splits) {
    float* ws = nullptr;
    const int splits = qs_append_split_resolve(wanted_splits, a, p, &ws);
    if (!ws) return qs_append_launch(a, p);      // one split, or no workspace (first use inside a capture): bit for bit qs_append_attention
    const int lrc = launch_kernel_pair<append_attention_split_kernel<true>, append_attention_split_kernel<false>>(
        "append_attention_split", "append_attention_split", a.int4, dim3(a.num_kv_heads, p.q_tiles * splits, a.batch), dim3(64 * p.waves), a.stream,
        a.qkv, ws, a.cu_seqlens_q, a.past_lens, a.kv_pointers, a.num_heads, a.num_kv_heads, a.max_blocks, p.tile_tokens, p.q_tiles, splits,
        a.qkv_stride0);
    return lrc != QS_OK ? lrc : qs_append_merge_launch(ws, a, p, splits);
}

extern "C" int qs_append_attention_split_plan(int batch, int max_seqlen_q, int max_past, int num_heads, int num_kv_heads,
                                              int int4_kv_cache, int* plan5) {
    QS_REQUIRE(plan5, "append attention split plan: null output");
    plan5[0] = plan5[1] = plan5[2] = plan5[3] = plan5[4] = 0;
    QS_REQUIRE(max_past >= 0, "append_attention_split: negative max_past");
    const int rc = qs_append_attention_plan(batch, max_seqlen_q, num_heads, num_kv_heads, plan5);   // (checks the rest, fills 0 .. 2)
    if (rc != QS_OK || plan5[1] == 0) return rc;
    (void)int4_kv_cache;                                 // both cache types walk 64-token pages: one rule
    const int splits = attn_plan::plan_splits(batch, plan5[1], num_kv_heads, max_past, qs_split_workspace_capacity());
    plan5[3] = splits;
    // KiB of partial records (a record block is 16 640 B, four per workgroup: 65 KiB); 0 for the un-split launch, which has none
    plan5[4] = splits > 1 ? (int)(attn_plan::append_split_bytes((size_t)batch * num_kv_heads * plan5[1]) * splits / 1024) : 0;
    return QS_OK;
}

extern "C" int qs_append_attention_split(const void* qkv, void* out, const int32_t* cu_seqlens_q, const int32_t* past_lens,
                                         const int64_t* kv_pointers, int num_tokens, int batch, int max_seqlen_q, int max_blocks,
                                         int num_heads, int num_kv_heads, int head_dim, int64_t qkv_stride0, int64_t out_stride0,
                                         int tokens_per_block, int size_per_token, int int4_kv_cache, int kv_cache_with_zeros,
                                         int max_past, int num_splits, qs_stream_t stream) {
    AppendArgs a;
    if (const int bad = check_append_args(qkv, out, cu_seqlens_q, past_lens, kv_pointers, num_tokens, batch, max_seqlen_q, max_blocks, num_heads,
                                          num_kv_heads, head_dim, qkv_stride0, out_stride0, tokens_per_block, size_per_token, int4_kv_cache,
                                          kv_cache_with_zeros, stream, &a); bad != QS_OK)
        return bad;
    QS_REQUIRE(num_splits >= 0, "append_attention_split: num_splits=%d (0 = ask the planner, >= 1 = forced)", num_splits);
    int plan5[5];
    const int rc = qs_append_attention_split_plan(batch, max_seqlen_q, table_hint(max_past, max_blocks), num_heads, num_kv_heads, int4_kv_cache, plan5);
    if (rc != QS_OK || a.empty()) return rc;
    return qs_append_split_launch(a, {plan5[0], plan5[1], plan5[2]}, num_splits > 0 ? num_splits : plan5[3]);
}
