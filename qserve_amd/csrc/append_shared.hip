// append_shared.hip -- shared-prefix append attention for MI355X (gfx950): the op of append_attention.hip for a batch whose sequences
// come in GROUPS of batch-adjacent members that hold the SAME leading pages (a system prompt, a few-shot header: the members' K / V
// table rows name the same pages for the first prefix / 64 entries).  The other entries walk those pages once per (sequence, KV head,
// query tile); here a group's new rows - one contiguous token range of the packed qkv buffer - ride on ONE walk of them.  DESIGN.md 10.
//
// Two launches on one stream (the split-KV entry's form: partial records in the split-KV workspace, no in-launch wait, no atomics):
//   1. append_shared_kernel<INT4>, grid (KV heads, y, groups + sequences); the role of a workgroup is uniform and chosen by z, the
//      group workgroups first (z < groups: the longer chains are dispatched first).  Both roles are ONE call of walk_keys with other
//      arguments:
//        * PREFIX role (group g, query tile of the group, prefix split s of P): the group's tokens cu_q[first] .. cu_q[last + 1] - 1 as
//          the rows of one sequence (row r = G * token + g of the tile, the mapping of every append kernel), pages
//          split_range(prefix, s, P) of the FIRST member's table, no new keys, nothing masked: every row sees every prefix key;
//        * SUFFIX role (sequence b, query tile, suffix split s of S): append_attention_split.hip's workgroup over the sequence's pages
//          from prefix / 64 on - the table and the past are counted from there -, the last split with the new tokens (causal).
//      A workgroup without a key range, without a token, or beyond its role's share of y returns at once and writes nothing.
//      prefix = prefix_lens[g] rounded DOWN to whole pages and cut to the pointer table; group bounds and group indices are cut to
//      the batch: whatever the arrays hold, no address outside the tables, the pages they name and the workspace is formed.
//   2. append_shared_merge_kernel, grid (KV heads, query tiles x 4, sequences) - the sequence mapping: per (token, head) the written
//      prefix records of the sequence's group, found through the GROUP mapping (gi = cu_q[b] - cu_q[first] + i: tile gi / tq, row
//      (gi % tq) * G + g, wave row / 32, lane row % 32), then the written suffix records, in key order, with the split merge's arithmetic
//      (M = max m, weights 2^(m - M), m = -inf weighs 0, no key = exactly 0, fp32 sums and divide, fp16 out).  "Written" is recomputed
//      from past_lens / prefix_lens / cu_q: stale workspace contents are never read as data.
//
// Workspace: the prefix records [group][group tile][KV head][P][rec_waves_prefix], then the suffix records [sequence][tile][KV head]
// [S][rec_waves_suffix], blocks of REC_FLOATS floats (append_attention_split.hip has the block's layout).  rec_waves = the waves of a
// workgroup that can own a row, known on the host: ceil(min(tq, max tokens of the role's "sequence") * G / 32), at most 4 - with the
// split entry's constant 4, B = 64 x 8 KV heads would need 33 MB for ONE set of suffix records, more than the 32 MiB workspace.
#include "append_walk.h"

namespace {

using namespace qs_flash;
using namespace qs_append;

using attn_plan::SharedPlan;      // the planner's rule: attn_plan.h plan_shared (qs_append_shared_plan reports it)

struct SharedGeom {
    int num_heads, num_kv_heads, max_blocks, batch, num_groups;
    int tq, q_tiles, gq_tiles, P, S, rw_prefix, rw_suffix;
    long suffix_off;                 // blocks of REC_FLOATS in front of the suffix records
};

// the whole-page prefix of group g, cut to the pointer table
__device__ __forceinline__ int group_prefix(const int* __restrict__ prefix_lens, int g, int max_blocks) { return clamp_past(prefix_lens[g], max_blocks) & ~(BN - 1); }
__device__ __forceinline__ int clamp_index(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }

template <bool INT4>
__global__ __launch_bounds__(64 * NWV, 2) void append_shared_kernel(const _Float16* __restrict__ qkv, float* __restrict__ ws,
                                                                   const int* __restrict__ cu_q, const int* __restrict__ past_lens,
                                                                   const int64_t* __restrict__ kv_pointers,
                                                                   const int* __restrict__ group_offsets, const int* __restrict__ prefix_lens,
                                                                   const int* __restrict__ seq_group, SharedGeom ge, int64_t qkv_stride0,
                                                                   float scale_log2) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hkv = blockIdx.x, y = blockIdx.y, z = blockIdx.z;
    const int G = ge.num_heads / ge.num_kv_heads;
    // ---- the role (workgroup-uniform): who the rows are, which pages are walked, where the records go
    int q_start, n, tok0, np, past, rw;
    bool with_new;
    const int64_t* ktab;
    long block0;                                          // the record block of wave 0
    if (z < ge.num_groups) {                              // PREFIX: the group's tokens over a range of the first member's prefix pages
        if (y >= ge.gq_tiles * ge.P) return;
        const int first = clamp_index(group_offsets[z], ge.batch), end = clamp_index(group_offsets[z + 1], ge.batch);
        if (end <= first) return;
        const int tile = y / ge.P, split = y % ge.P;
        q_start = cu_q[first], n = cu_q[end] - q_start;
        tok0 = tile * ge.tq;
        if (tok0 >= n) return;
        const PageRange pr = split_range(group_prefix(prefix_lens, z, ge.max_blocks), split, ge.P);
        if (pr.np == 0) return;                           // EMPTY: no record (the merge recomputes this test)
        np = pr.np, past = pr.np * BN, with_new = false;  // whole pages: no slot masked, no causal limit
        ktab = kv_pointers + (size_t)first * 2 * ge.max_blocks + pr.p0;
        rw = ge.rw_prefix;
        block0 = ((((long)z * ge.gq_tiles + tile) * ge.num_kv_heads + hkv) * ge.P + split) * rw;
    } else {                                              // SUFFIX: the split kernel's workgroup behind the prefix pages
        if (y >= ge.q_tiles * ge.S) return;
        const int b = z - ge.num_groups;
        const int split = y % ge.S, qt = ge.q_tiles - 1 - y / ge.S;
        q_start = cu_q[b], n = cu_q[b + 1] - q_start;
        tok0 = qt * ge.tq;
        if (tok0 >= n) return;
        const int prefix = group_prefix(prefix_lens, clamp_index(seq_group[b], ge.num_groups - 1), ge.max_blocks);
        const int own = clamp_past(past_lens[b], ge.max_blocks) - prefix;      // (< 0: a violated precondition - the rows are unspecified)
        const int past_sfx = own < 0 ? 0 : own;
        const PageRange pr = split_range(past_sfx, split, ge.S);
        with_new = split == ge.S - 1;
        if (pr.np == 0 && !with_new) return;
        np = pr.np, past = past_sfx - pr.p0 * BN;
        ktab = kv_pointers + (size_t)b * 2 * ge.max_blocks + prefix / BN + pr.p0;
        rw = ge.rw_suffix;
        block0 = ge.suffix_off + ((((long)b * ge.q_tiles + qt) * ge.num_kv_heads + hkv) * ge.S + split) * rw;
    }

    v16f oacc[4];
    float m_run, l_run;
    if (!walk_keys<INT4>(smem, qkv, ktab, ktab + ge.max_blocks, ge.num_heads, ge.num_kv_heads, hkv, G, q_start, n, tok0, ge.tq, np, past, with_new,
                         qkv_stride0, scale_log2, CausalNewKeys(), lane, wave, oacc, m_run, l_run))
        return;                                          // (behind the last barrier; the merge skips this wave's block by the same test)
    if (wave >= rw) return;                              // (only with more tokens than the host announced: no block of its own)
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    store_partial_record(ws + (size_t)(block0 + wave) * REC_FLOATS, oacc, m_run, l_tot);
}

// One workgroup per (KV head, query tile, wave block of 32 rows, sequence) - append_attention_merge_kernel's mapping; thread (row
// li = tid & 31, tid >> 5) merges the chunks (tid >> 5) + 8 i, i = 0 .. 3, of its row over the written prefix, then suffix records.
__global__ __launch_bounds__(256) void append_shared_merge_kernel(const float* __restrict__ ws, _Float16* __restrict__ out,
                                                                 const int* __restrict__ cu_q, const int* __restrict__ past_lens,
                                                                 const int* __restrict__ group_offsets, const int* __restrict__ prefix_lens,
                                                                 const int* __restrict__ seq_group, SharedGeom ge, int64_t o_stride0) {
    const int hkv = blockIdx.x, b = blockIdx.z;
    const int qt = (int)blockIdx.y / NWV, wave = (int)blockIdx.y % NWV;
    const int G = ge.num_heads / ge.num_kv_heads, tq = ge.tq;
    const int q_start = cu_q[b], n = cu_q[b + 1] - q_start;
    const int tok0 = qt * tq;
    if (tok0 >= n || wave * 32 >= tq * G || tok0 + (wave * 32) / G >= n || wave >= ge.rw_suffix) return;   // no record: the kernel's tests
    const int li = threadIdx.x & 31, c0 = threadIdx.x >> 5;
    const int r = wave * 32 + li, tok = tok0 + r / G;
    if (r >= tq * G || tok >= n) return;                 // a row of the block without a token
    // ---- the suffix records: the sequence mapping
    const int g = clamp_index(seq_group[b], ge.num_groups - 1);
    const int prefix = group_prefix(prefix_lens, g, ge.max_blocks);
    const int own = clamp_past(past_lens[b], ge.max_blocks) - prefix;
    const int np_s = ((own < 0 ? 0 : own) + BN - 1) / BN;
    const int pps_s = (np_s + ge.S - 1) / ge.S;
    const float* const srec0 = ws + (size_t)(ge.suffix_off + ((((long)b * ge.q_tiles + qt) * ge.num_kv_heads + hkv) * ge.S) * ge.rw_suffix + wave) * REC_FLOATS;
    const size_t sstep = (size_t)ge.rw_suffix * REC_FLOATS;
    auto swritten = [&](int s) { return s * pps_s < np_s || s == ge.S - 1; };
    // ---- the prefix records: the group mapping
    const int first = clamp_index(group_offsets[g], ge.batch), end = clamp_index(group_offsets[g + 1], ge.batch);
    const int gi = end > first ? q_start - cu_q[first] + tok : -1;
    const int n_group = end > first ? cu_q[end] - cu_q[first] : 0;
    const int gtile = gi >= 0 ? gi / tq : 0, grow = gi >= 0 ? (gi % tq) * G + r % G : 0;
    const int gwave = grow / 32, gli = grow % 32;
    const bool has_prefix = gi >= 0 && gi < n_group && gtile < ge.gq_tiles && gwave < ge.rw_prefix;
    const int np_p = has_prefix ? prefix / BN : 0;
    const int pps_p = (np_p + ge.P - 1) / ge.P;
    const float* const prec0 = ws + (size_t)(((((long)g * ge.gq_tiles + gtile) * ge.num_kv_heads + hkv) * ge.P) * ge.rw_prefix + gwave) * REC_FLOATS;
    const size_t pstep = (size_t)ge.rw_prefix * REC_FLOATS;
    auto pwritten = [&](int s) { return s * pps_p < np_p; };

    float M = -INFINITY;
    for (int s = 0; s < ge.P; ++s)
        if (pwritten(s)) M = fmaxf(M, prec0[s * pstep + 32 * DH + gli]);
    for (int s = 0; s < ge.S; ++s)
        if (swritten(s)) M = fmaxf(M, srec0[s * sstep + 32 * DH + li]);
    v4f acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = (v4f){0.f, 0.f, 0.f, 0.f};
    float den = 0.f;
    auto add = [&](const float* rec, int l) {
        const float m = rec[32 * DH + l];
        if (m == -INFINITY) return;                      // the range saw no key of this row: l = 0, O = 0 (and M may be -inf too)
        const float w = __builtin_amdgcn_exp2f(m - M);
        den += w * rec[32 * DH + 32 + l];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] += w * *reinterpret_cast<const v4f*>(rec + (c0 + 8 * i) * 128 + l * 4);
    };
    for (int s = 0; s < ge.P; ++s)
        if (pwritten(s)) add(prec0 + s * pstep, gli);
    for (int s = 0; s < ge.S; ++s)
        if (swritten(s)) add(srec0 + s * sstep, li);
    const float inv = den > 0.f ? 1.0f / den : 0.f;       // no key at all: exactly 0
    _Float16* const orow = out + (size_t)(q_start + tok) * o_stride0 + (size_t)(hkv * G + r % G) * DH;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const h4 o = {(_Float16)(acc[i][0] * inv), (_Float16)(acc[i][1] * inv), (_Float16)(acc[i][2] * inv), (_Float16)(acc[i][3] * inv)};
        *reinterpret_cast<h4*>(orow + (c0 + 8 * i) * 4) = o;
    }
}

int check_shared_sizes(int batch, int max_seqlen_q, int num_groups, int max_group_tokens, int num_heads, int num_kv_heads) {
    QS_REQUIRE(batch >= 0 && max_seqlen_q >= 0 && num_groups >= 0 && max_group_tokens >= 0,
               "append_attention_shared: negative batch / max_seqlen_q / num_groups / max_group_tokens");
    QS_REQUIRE(batch == 0 || (num_groups >= 1 && num_groups <= batch), "append_attention_shared: num_groups=%d not in 1..batch=%d", num_groups, batch);
    QS_REQUIRE(num_heads > 0 && num_kv_heads > 0 && num_heads % num_kv_heads == 0, "append_attention_shared: bad head counts H=%d Hkv=%d", num_heads,
               num_kv_heads);
    if (num_heads / num_kv_heads > MAX_G) {
        qs_set_error("append_attention_shared: num_heads/num_kv_heads = %d not in 1..%d", num_heads / num_kv_heads, MAX_G);
        return QS_ENOSUP;
    }
    return QS_OK;
}

// the shared launch and its merge; no workspace (its first use inside a capture): the un-split launch - correct because the members'
// prefix entries are equal
int shared_launch(const AppendArgs& a, const int32_t* group_offsets, const int32_t* prefix_lens, const int32_t* seq_group, int num_groups,
                  const SharedPlan& p) {
    const AppendPlan ap = {p.tq, p.q_tiles, p.waves};
    float* const ws = qs_split_workspace(p.bytes, a.stream);
    if (!ws) return qs_append_launch(a, ap);
    SharedGeom ge;
    ge.num_heads = a.num_heads, ge.num_kv_heads = a.num_kv_heads, ge.max_blocks = a.max_blocks, ge.batch = a.batch, ge.num_groups = num_groups;
    ge.tq = p.tq, ge.q_tiles = p.q_tiles, ge.gq_tiles = p.gq_tiles, ge.P = p.P, ge.S = p.S, ge.rw_prefix = p.rw_prefix, ge.rw_suffix = p.rw_suffix;
    ge.suffix_off = (long)num_groups * p.gq_tiles * a.num_kv_heads * p.P * p.rw_prefix;
    const int ny = p.gq_tiles * p.P > p.q_tiles * p.S ? p.gq_tiles * p.P : p.q_tiles * p.S;
    QS_REQUIRE(ny <= 65535 && num_groups + a.batch <= 65535, "append_attention_shared: the grid (%d, %d) exceeds the launch limits", ny,
               num_groups + a.batch);
    const int lrc = launch_kernel_pair<append_shared_kernel<true>, append_shared_kernel<false>>(
        "append_attention_shared", "append_attention_shared", a.int4, dim3(a.num_kv_heads, ny, num_groups + a.batch), dim3(64 * p.waves), a.stream,
        a.qkv, ws, a.cu_seqlens_q, a.past_lens, a.kv_pointers, group_offsets, prefix_lens, seq_group, ge, a.qkv_stride0);
    if (lrc != QS_OK) return lrc;
    hipLaunchKernelGGL(append_shared_merge_kernel, dim3(a.num_kv_heads, p.q_tiles * NWV, a.batch), dim3(256), 0, a.stream, ws, a.out, a.cu_seqlens_q,
                       a.past_lens, group_offsets, prefix_lens, seq_group, ge, a.out_stride0);
    return qs_launch_status("append_shared_merge");
}

}  // namespace

extern "C" int qs_append_shared_plan(int batch, int max_seqlen_q, int num_groups, int max_group_tokens, int max_prefix, int max_suffix_past,
                                     int num_heads, int num_kv_heads, int int4_kv_cache, int* plan8) {
    QS_REQUIRE(plan8, "append shared plan: null output");
    for (int i = 0; i < 8; ++i) plan8[i] = 0;
    if (const int rc = check_shared_sizes(batch, max_seqlen_q, num_groups, max_group_tokens, num_heads, num_kv_heads); rc != QS_OK) return rc;
    QS_REQUIRE(max_prefix >= 0 && max_suffix_past >= 0, "append_attention_shared: negative max_prefix / max_suffix_past");
    if (batch == 0 || max_seqlen_q == 0 || max_group_tokens == 0) return QS_OK;
    const SharedPlan p = attn_plan::plan_shared(batch, max_seqlen_q, num_groups, max_group_tokens, max_prefix, max_suffix_past, num_heads,
                                                num_kv_heads, 0, 0, qs_split_workspace_capacity());
    plan8[0] = p.tq, plan8[1] = p.q_tiles, plan8[2] = p.waves, plan8[4] = p.gq_tiles, plan8[5] = p.P;
    if (p.P == 0) {                                      // the split entry's launch over the whole past
        int plan5[5];
        const long whole = (long)max_prefix + max_suffix_past;
        const int rc = qs_append_attention_split_plan(batch, max_seqlen_q, whole > INT32_MAX ? INT32_MAX : (int)whole, num_heads, num_kv_heads,
                                                      int4_kv_cache, plan5);
        if (rc != QS_OK) return rc;
        plan8[3] = plan5[3], plan8[6] = NWV, plan8[7] = plan5[4];
        return QS_OK;
    }
    plan8[3] = p.S;
    plan8[6] = p.rw_suffix | (p.rw_prefix << 8);
    plan8[7] = (int)((p.bytes + 1023) / 1024);
    return QS_OK;
}

extern "C" int qs_append_attention_shared(const void* qkv, void* out, const int32_t* cu_seqlens_q, const int32_t* past_lens,
                                          const int64_t* kv_pointers, const int32_t* group_offsets, const int32_t* prefix_lens,
                                          const int32_t* seq_group, int num_tokens, int batch, int num_groups, int max_seqlen_q,
                                          int max_group_tokens, int max_blocks, int num_heads, int num_kv_heads, int head_dim,
                                          int64_t qkv_stride0, int64_t out_stride0, int tokens_per_block, int size_per_token, int int4_kv_cache,
                                          int kv_cache_with_zeros, int max_prefix, int max_suffix_past, int num_prefix_splits,
                                          int num_suffix_splits, qs_stream_t stream) {
    AppendArgs a;
    if (const int bad = check_append_args(qkv, out, cu_seqlens_q, past_lens, kv_pointers, num_tokens, batch, max_seqlen_q, max_blocks, num_heads,
                                          num_kv_heads, head_dim, qkv_stride0, out_stride0, tokens_per_block, size_per_token, int4_kv_cache,
                                          kv_cache_with_zeros, stream, &a); bad != QS_OK)
        return bad;
    QS_REQUIRE(group_offsets && prefix_lens && seq_group, "append_attention_shared: null group array");
    if (const int rc = check_shared_sizes(batch, max_seqlen_q, num_groups, max_group_tokens, num_heads, num_kv_heads); rc != QS_OK) return rc;
    QS_REQUIRE(num_prefix_splits >= -1, "append_attention_shared: num_prefix_splits=%d (0 = ask the planner, >= 1 = forced, -1 = do not share)",
               num_prefix_splits);
    QS_REQUIRE(num_suffix_splits >= 0, "append_attention_shared: num_suffix_splits=%d (0 = ask the planner, >= 1 = forced)", num_suffix_splits);
    if (a.empty() || max_group_tokens == 0) return QS_OK;
    const int hint_p = table_hint(max_prefix, max_blocks), hint_s = table_hint(max_suffix_past, max_blocks);
    const size_t capacity = qs_split_workspace_capacity();
    const SharedPlan p = attn_plan::plan_shared(batch, max_seqlen_q, num_groups, max_group_tokens, hint_p, hint_s, num_heads, num_kv_heads,
                                                num_prefix_splits, num_suffix_splits, capacity);
    if (p.P != 0) return shared_launch(a, group_offsets, prefix_lens, seq_group, num_groups, p);
    // do not share: the split launch over the whole past (its planner, or the forced count)
    const int planned = attn_plan::plan_splits(batch, p.q_tiles, num_kv_heads, table_hint(hint_p + hint_s, max_blocks), capacity);
    return qs_append_split_launch(a, {p.tq, p.q_tiles, p.waves}, num_suffix_splits > 0 ? num_suffix_splits : planned);
}
