// attention_long.hip -- decode attention for page tables of ANY length on the matrix cores (gfx950): split-KV over page ranges that
// are cut on the device, for chains that are long and grids that are small (one sequence of 131 072 tokens is 8 (sequence, KV head)
// pairs on 256 CUs).  The contract is qs_single_query_attention's: rotate q and the new k, quantise the new token's k / v into its
// page slot (kv_quant.h: the same bits), attend over the cached tokens plus the new one.  KV4 and KV8, G = H / Hkv in 1 .. 8.
//
// Mapping
//   * workgroup = (KV head, sequence, range), grid (Hkv, batch, S).  S is the host's (attn_plan.h plan_decode_long, from the table's
//     length): a captured graph keeps its grid while the lengths grow.  The RANGE is cut here from lengths[b]: the sequence's
//     npages = ceil((length - 1) / 64) cached pages go evenly to nr = clamp(npages / min_pages, 1, S) ranges, range z = pages
//     [z npages / nr, (z + 1) npages / nr); a workgroup with z >= nr writes an empty record (maximum -3e38, sum 0, O = 0) and exits.
//     A short text under a long table is a few short chains; nothing crosses to the host.
//   * range nr - 1 ends at the sequence's last page: it ALONE quantises and writes the new token (wave 0: K, wave 1: V) and adds the
//     new token's own term (fp32 q.k of the rotated fp16 rows, the un-quantised v) to its result, as the other decode kernels do.
//   * 4 waves; wave w owns pages begin + w, begin + w + 4, ... of the range as whole pages and needs no barrier while it walks them.
//     One wave per SIMD; a page is 16 + 16 MFMAs behind 32 de-quantisations of 8 values per lane and the regrouping of P.V's
//     operands, about 1 100 instructions per page and wave: KV8 runs within 1.2 x of its bytes' time at 6.29 TB/s, KV4 at 1.5 x -
//     its walk, not the DMA, is the bound (profiles/decode_long.txt) -, and eight pages in flight per workgroup keep the requests
//     coming.  Half-page units would halve the LDS and double the waits per byte: not taken.
// Data movement
//   * page ADDRESSES are staged per range, not per sequence: a window of WIN = 256 K and 256 V addresses in LDS, refilled as the
//     range walks (two barriers per 256 pages, the rings drained across them - about 1 % of a window's 256 pages x 0.34 us / 4
//     waves).  The table is limited by nothing but max_blocks; S = 1 over 2 048 pages is eight windows.
//   * K and V pages travel HBM -> LDS by LDS-DMA (global_load_lds, 16 B per lane, non-temporal: every byte is read once per step)
//     into a wave-private ring of DEPTH = 2 stages of [K page | V page | k scale, k zero, v scale, v zero]; a stage is 10 (KV4) /
//     18 (KV8) VMEM instructions, waited for with counted vmcnt: vmcnt(NVM) while the next page is in flight, vmcnt(0) at a tail.
//   * LDS images are made conflict-free on the DMA's SOURCE side: KV8 K rows hold 16-byte chunk c at position c ^ ((row >> 1) & 7)
//     (a b128 read of 16 rows at 128 B stride then covers all banks); V tokens sit in slot (t & ~3) | ((t + (t >> 2)) & 3), so the
//     four rows 4 tg + r that the four lane groups read together land in four different quarters of 256 B.  KV4 K needs nothing (a
//     tile's 16 rows x 64 B are 1 KiB contiguous).
//   * de-quantisation runs in registers between ds_read and the MFMA operand, with append_dequant.h's dequant8 (the decode kernels'
//     exact values: scale and zero applied per token, rounded to fp16) - 8 consecutive dims of a token are one A operand of Q.K^T;
//     for P.V a lane de-quantises 8 dims of each of its 8 tokens and regroups them in registers into 8 operands of 8 tokens.
// Arithmetic (v_mfma_f32_16x16x32_f16, all G heads from one read of a page)
//   * S^T[token][head] = K q^T: A = 16 tokens x 32 dims, B = rotated q (rows >= G zero, held in registers for the whole walk); lane
//     (li, tg) receives tokens 16 t + 4 tg + r of head li - exactly the 8 + 8 tokens it supplies as B operand of
//     O^T[dim][head] = V^T P^T per half page, so the probabilities never change lanes.  Online softmax in the log2 domain, fp32
//     maxima and sums (the sums of the un-rounded probabilities; the operand is their fp16 rounding).
//   * waves merge through LDS (the dead rings); S = 1 normalises and stores `out`, S > 1 writes one record O[128], m, l per head in
//     attn_plan::decode_split_bytes' layout and qs_launch_attention_merge (attention_mfma.hip) combines them in range order: no
//     cross-workgroup wait inside the launch, results bit-identical run to run and under graph replay.
// LDS: KV4 2 x 4 x (8 KiB + 512) = 68 KiB of rings, KV8 132 KiB; + 4 KiB q, 4 KiB window, < 1 KiB of scalars: 78 / 142 KiB of 160.
// The workgroup's statements are attention_long_body.h, shared as text with the sliding-window kernels of attention_window.hip.
#include "attention_long_walk.h"

namespace {

using namespace qs_long;

template <bool INT4>
__global__ __launch_bounds__(TPB) void decode_long_kernel(
    const _Float16* __restrict__ q, const _Float16* __restrict__ k, const _Float16* __restrict__ v,
    const int64_t* __restrict__ kv_pointers, const int* __restrict__ lengths, _Float16* __restrict__ out, int num_heads,
    int num_kv_heads, int G, int64_t q_stride0, int64_t kv_stride0, int max_blocks, int timestep, float rope_base,
    const float2* __restrict__ rope_tab, int rope_tab_len, int S, int min_pages, float* __restrict__ ws) {
    constexpr bool WINDOW = false;
    constexpr int window = 0;
#include "attention_long_body.h"
}

int single_query_attention_long(const void* q, const void* k, const void* v, const int64_t* kv_pointers, const int32_t* length_per_sample,
                                void* out, int batch, int num_heads, int num_kv_heads, int head_dim, int64_t q_stride0, int64_t kv_stride0,
                                int max_blocks, int memory_max_seqlen, int tokens_per_block, int size_per_token, int timestep,
                                int rotary_embedding_dim, float rotary_base, int int4_kv_cache, int kv_cache_with_zeros, int num_splits,
                                qs_stream_t stream) {
    DecodeLongArgs a;
    if (const int bad = check_decode_long_args("single_query_attention_long", q, k, v, kv_pointers, length_per_sample, out, batch, num_heads,
                                               num_kv_heads, head_dim, q_stride0, kv_stride0, max_blocks, memory_max_seqlen, tokens_per_block,
                                               size_per_token, timestep, rotary_embedding_dim, rotary_base, int4_kv_cache, kv_cache_with_zeros,
                                               num_splits, stream, &a); bad != QS_OK)
        return bad;
    if (batch == 0) return QS_OK;
    LongPlan plan = attn_plan::plan_decode_long(batch, num_kv_heads, a.d.G, max_blocks, a.int4, qs_split_workspace_capacity());
    if (num_splits >= 1) plan.splits = num_splits > attn_plan::MAX_SPLITS ? attn_plan::MAX_SPLITS : num_splits;
    return qs_launch_decode_long(a, plan);
}

}  // namespace

int qs_launch_decode_long(const DecodeLongArgs& a, const LongPlan& plan) {
    return launch_long_kernels<decode_long_kernel<true>, decode_long_kernel<false>>("single_query_attention_long", a, plan);
}

extern "C" int qs_single_query_attention_long(const void* q, const void* k, const void* v, const int64_t* kv_pointers,
                                              const int32_t* length_per_sample, void* out, int batch, int num_heads, int num_kv_heads,
                                              int head_dim, int64_t q_stride0, int64_t kv_stride0, int max_blocks, int memory_max_seqlen,
                                              int tokens_per_block, int size_per_token, int timestep, int rotary_embedding_dim,
                                              float rotary_base, int neox_rotary_style, int int4_kv_cache, int kv_cache_with_zeros,
                                              int num_splits, qs_stream_t stream) {
    (void)neox_rotary_style;       // accepted, no effect: as in qs_single_query_attention
    return single_query_attention_long(q, k, v, kv_pointers, length_per_sample, out, batch, num_heads, num_kv_heads, head_dim, q_stride0,
                                       kv_stride0, max_blocks, memory_max_seqlen, tokens_per_block, size_per_token, timestep,
                                       rotary_embedding_dim, rotary_base, int4_kv_cache, kv_cache_with_zeros, num_splits, stream);
}

extern "C" int qs_single_query_attention_long_plan(int batch, int num_heads, int num_kv_heads, int max_blocks, int int4_kv_cache,
                                                   int* plan3) {
    QS_REQUIRE(plan3, "single_query_attention_long plan: null output");
    plan3[0] = plan3[1] = plan3[2] = 0;
    QS_REQUIRE(batch >= 0 && num_heads > 0 && num_kv_heads > 0 && num_heads % num_kv_heads == 0,
               "single_query_attention_long: bad head counts H=%d Hkv=%d", num_heads, num_kv_heads);
    QS_REQUIRE(max_blocks > 0, "single_query_attention_long: bad max_blocks / memory_max_seqlen");
    if (num_heads / num_kv_heads > 8) {
        qs_set_error("single_query_attention_long: num_heads/num_kv_heads = %d not in 1..8", num_heads / num_kv_heads);
        return QS_ENOSUP;
    }
    if (batch == 0) return QS_OK;
    const LongPlan p = attn_plan::plan_decode_long(batch, num_kv_heads, num_heads / num_kv_heads, max_blocks, int4_kv_cache != 0,
                                                   qs_split_workspace_capacity());
    plan3[0] = p.splits, plan3[1] = p.waves, plan3[2] = p.min_pages;
    return QS_OK;
}
