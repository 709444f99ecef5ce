// attn_host.h -- the host layer the attention translation units share: the library-managed scratch of attention_mfma.hip, one
// argument record per entry family, and the launchers that take a record and a plan of attn_plan.h.  Declarations only (and the
// argument checks that fill a record); every definition lives in the file named next to it.
#pragma once
#include "attn_plan.h"
#include "common.h"

// ---- library-managed scratch (attention_mfma.hip) ----------------------------------------------------------------------------
float* qs_split_workspace(size_t bytes, hipStream_t st);     // nullptr: beyond the capacity, or its first use inside a capture
size_t qs_split_workspace_capacity();
const float2* qs_rope_table(float base, int max_pos, hipStream_t st, int* len_out);
unsigned* qs_attn_quant_counters(hipStream_t st, int batch);
// second phase of the decode kernels' split-KV, shared with the KV8 kernel (attention_mfma8.hip)
void qs_launch_attention_merge(const float* ws, _Float16* out, int H, int Hkv, int G, int nsplit, int batch, hipStream_t st);

// ---- decode attention: what single_query_attention (attention.hip) hands the launcher its plan names ---------------------------
struct DecodeArgs {
    int G;                           // num_heads / num_kv_heads
    dim3 grid;                       // (KV heads, sequences); the launchers add the splits
    hipStream_t st;
    const _Float16 *q, *k, *v;
    const int64_t* kvp;
    const int* len;
    _Float16* out;
    int H, Hkv;
    int64_t qs, kvs;                 // token strides of q and of k / v
    int mb, timestep;
    float base;
    int max_pos;                     // memory_max_seqlen: the length asked of the RoPE table
    const QsAttnQuant* quant;        // nullable: qs_single_query_attention_quant's request, *fused = whether the launch finished
    bool* fused;                     // the quantised row as well (the KV4 launcher only)
};
// the record's fields under the names the launchers' QS_LAUNCH_G switches use (grid is the launcher's own copy: it adds the splits)
#define QS_DECODE_LOCALS(a)                                                                                         \
    const int G = (a).G, H = (a).H, Hkv = (a).Hkv, mb = (a).mb, timestep = (a).timestep, max_pos = (a).max_pos;     \
    dim3 grid = (a).grid;                                                                                           \
    hipStream_t st = (a).st;                                                                                        \
    const _Float16 *q = (a).q, *k = (a).k, *v = (a).v;                                                              \
    const int64_t *kvp = (a).kvp, qs = (a).qs, kvs = (a).kvs;                                                       \
    const int* len = (a).len;                                                                                       \
    _Float16* out = (a).out;                                                                                        \
    const float base = (a).base
int qs_launch_decode_mfma(const DecodeArgs& a, const attn_plan::AttnPlan& plan);    // family 1, attention_mfma.hip
int qs_launch_decode_mfma8(const DecodeArgs& a, const attn_plan::AttnPlan& plan);   // family 2, attention_mfma8.hip

// ---- append attention: the four entries' common arguments, checked ------------------------------------------------------------
struct AppendArgs {
    const _Float16* qkv;
    _Float16* out;
    const int32_t *cu_seqlens_q, *past_lens;
    const int64_t* kv_pointers;
    const uint64_t* tree_mask;       // the tree entry's; nullptr elsewhere
    int num_tokens, batch, max_seqlen_q, max_blocks, num_heads, num_kv_heads;
    int64_t qkv_stride0, out_stride0;
    bool int4;
    hipStream_t stream;
    bool empty() const { return batch == 0 || max_seqlen_q == 0 || num_tokens == 0; }      // nothing to do: no launch
};
// The layout contract of the attention entries (include/qserve_amd.h), checked before any device call - the ONE statement of it:
// every append entry asks here, once, and works on the record from then on (the group size is checked by the plan entries).
inline int check_append_args(const void* qkv, void* out, const int32_t* cu_seqlens_q, const int32_t* past_lens, const int64_t* kv_pointers,
                             int num_tokens, int batch, int max_seqlen_q, int max_blocks, int num_heads, int num_kv_heads, int head_dim,
                             int64_t qkv_stride0, int64_t out_stride0, int tokens_per_block, int size_per_token, int int4_kv_cache,
                             int kv_cache_with_zeros, qs_stream_t stream, AppendArgs* a) {
    using attn_plan::DH;
    QS_REQUIRE(qkv && out && cu_seqlens_q && past_lens && kv_pointers, "append_attention: null pointer");
    QS_REQUIRE(num_tokens >= 0 && batch >= 0 && max_seqlen_q >= 0 && max_blocks > 0, "append_attention: bad sizes");
    QS_REQUIRE(num_heads > 0 && num_kv_heads > 0 && num_heads % num_kv_heads == 0,
               "append_attention: bad head counts H=%d Hkv=%d", num_heads, num_kv_heads);
    if (head_dim != DH || tokens_per_block != attn_plan::PAGE || !kv_cache_with_zeros) {
        qs_set_error("append_attention: only head_dim=128, tokens_per_block=64 and zero-point KV caches are supported");
        return QS_ENOSUP;
    }
    QS_REQUIRE(size_per_token == num_kv_heads * (int4_kv_cache ? DH / 2 : DH), "append_attention: size_per_token=%d, expected %d",
               size_per_token, num_kv_heads * (int4_kv_cache ? DH / 2 : DH));
    QS_REQUIRE(qkv_stride0 >= (int64_t)(num_heads + 2 * num_kv_heads) * DH && qkv_stride0 % 8 == 0 && qkv_stride0 < (1 << 24) &&
                   out_stride0 >= (int64_t)num_heads * DH && out_stride0 % 8 == 0,
               "append_attention: token strides must hold a row and keep 16-byte alignment");
    QS_REQUIRE((reinterpret_cast<uintptr_t>(qkv) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0,
               "append_attention: qkv and out must be 16-byte aligned");
    *a = {(const _Float16*)qkv, (_Float16*)out, cu_seqlens_q, past_lens, kv_pointers, nullptr, num_tokens, batch, max_seqlen_q, max_blocks,
          num_heads, num_kv_heads, qkv_stride0, out_stride0, int4_kv_cache != 0, (hipStream_t)stream};
    return QS_OK;
}
// a length hint of an entry, cut to the pointer table (a past is cut to the table anyway; negative = unknown = the table)
inline int table_hint(int hint, int max_blocks) {
    const int table = max_blocks * attn_plan::PAGE;
    return hint < 0 || hint > table ? table : hint;
}

// The launchers behind the entries: a checked record and its plan (no entry is re-entered to fall back).
// un-split: one workgroup per (sequence, KV head, query tile) walks the whole past (append_attention.hip)
int qs_append_launch(const AppendArgs& a, const attn_plan::AppendPlan& p);
// split-KV with merge for a wanted split count; one split, or no workspace (its first use inside a capture): qs_append_launch
// (append_attention_split.hip)
int qs_append_split_launch(const AppendArgs& a, const attn_plan::AppendPlan& p, int wanted_splits);
// qs_append_split_resolve: the effective split count for a wanted one - at most 64 and what the workspace holds - and the workspace
// for it; 1 and *ws = nullptr where the call has to run un-split.  qs_append_merge_launch: the merge of the partial records
// (mask-agnostic: it sees maxima, sums and O only).  Both in append_attention_split.hip; append_tree.hip is the other user.
int qs_append_split_resolve(int wanted, const AppendArgs& a, const attn_plan::AppendPlan& p, float** ws);
int qs_append_merge_launch(const float* ws, const AppendArgs& a, const attn_plan::AppendPlan& p, int splits);
