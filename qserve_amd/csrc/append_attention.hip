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
#include "append_dequant.h"

namespace {

using namespace qs_flash;
using namespace qs_append;      // the leaves shared with the split-KV kernels (append_attention_split.hip)

template <bool INT4>
__global__ __launch_bounds__(64 * NWV, 2) void append_attention_kernel(const _Float16* __restrict__ qkv, _Float16* __restrict__ out,
                                                                      const int* __restrict__ cu_q, const int* __restrict__ past_lens,
                                                                      const int64_t* __restrict__ kv_pointers, int num_heads,
                                                                      int num_kv_heads, int max_blocks, int tq, int64_t qkv_stride0,
                                                                      int64_t o_stride0, float scale_log2) {
    constexpr int DHB = INT4 ? DH / 2 : DH;        // bytes per cached token and head
    constexpr int NQ = INT4 ? 1 : 2;               // 16-byte loads per thread, page and tensor
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint8_t* const s_k = smem;                           // [2][16 KiB]  } the tile images of flash_tile.h
    uint8_t* const s_vt = smem + 2 * KS_BYTES;           // [2][16 KiB]  }

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // grid = (KV heads, query tiles, sequences); the query tiles of a sequence run last-to-first (the ones with the most keys first)
    const int hkv = blockIdx.x, qt = (int)(gridDim.y - 1 - blockIdx.y), b = blockIdx.z;
    const int G = num_heads / num_kv_heads;
    const int q_start = cu_q[b], n = cu_q[b + 1] - q_start;
    const int tok0 = qt * tq;                            // first new token of this tile
    if (tok0 >= n) return;                               // (n = 0: nothing read, nothing written)
    int past = past_lens[b];
    past = past < 0 ? 0 : past > max_blocks * BN ? max_blocks * BN : past;   // never walk beyond the pointer table
    const int np = (past + BN - 1) / BN;                 // phase 1: pages
    const int nk_new = n < tok0 + tq ? n : tok0 + tq;    // phase 2: new keys 0 .. nk_new - 1 are visible to some row
    const int nn = (nk_new + BN - 1) / BN;
    const int ntiles = np + nn;

    const int li = lane & 31, hi = lane >> 5;
    const int r_w = wave * 32 + li;                      // this lane's row (both lane halves share it)
    const int tok_r = tok0 + r_w / G;                    // its token; rows >= tq * G and tokens >= n compute, but are never stored
    const int tok_ld = tok_r < n ? tok_r : n - 1;

    // ---- Q fragments: B operand of S^T = K Q^T, lane (row, hi) holds dims 16s + 8hi .. +8 ----------------------------
    h8 qf[8];
    {
        const _Float16* qp = qkv + (size_t)(q_start + tok_ld) * qkv_stride0 + (size_t)(hkv * G + r_w % G) * DH + 8 * hi;
#pragma unroll
        for (int s = 0; s < 8; ++s) qf[s] = *reinterpret_cast<const h8*>(qp + 16 * s);
    }

    // ---- phase 2 staging by LDS-DMA (stage_fp16_tile): the new tokens' k / v rows of this KV head in the packed qkv buffer
    const _Float16* kg = qkv + (size_t)q_start * qkv_stride0 + (size_t)(num_heads + hkv) * DH;
    const TileRows ksrc = k_rows(kg, qkv_stride0, lane);
    const TileRows vsrc = v_rows(kg + (size_t)num_kv_heads * DH, qkv_stride0, lane);
    const u32 lds_k = lds_address(smem), lds_v = lds_k + 2 * KS_BYTES;
    auto load_new = [&](int j, int buf) { stage_fp16_tile(j, buf, n, wave, lds_k, ksrc, vsrc); };

    // ---- phase 1 staging: this head's [64 tokens][DHB bytes] slice of a page is contiguous.  Wave w owns tokens 16w .. 16w+15 of the
    // page - thread (token 16w + (lane >> 2), quarter lane & 3) de-quantises dims 32 quarter .. + 31 of K and of V - and the tile rows
    // 16w .. 16w+15 they become.  The raw bytes need no registers and no LDS of their own: the wave's LDS-DMA drops them (lane-linear)
    // into ITS OWN 4 KiB of the target K / V images while tile t is computed, and behind the P.V products every lane reads its
    // pieces back and writes the fp16 chunks over them.  Nobody else touches those rows before the barrier, and the LDS serves a
    // wave's accesses in order (the reads are complete - their data feeds the writes).  Scale / zero of the 16 tokens: two 4-byte
    // DMAs per page pair (lanes 0-7 scales, 8-15 zeros, the other lanes repeat them).
    const int64_t* ktab = kv_pointers + (size_t)b * 2 * max_blocks;
    const int64_t* vtab = ktab + max_blocks;
    constexpr int RAW_META = 2048;                       // raw data at + 0 (1 KiB KV4 / 2 KiB KV8), the parameters behind it
    auto dma4 = [&](u32 voff, const void* sbase, u32 lds_addr) {
        asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %0, %1" ::"v"(voff), "s"(sbase), "s"(lds_addr) : "memory");
    };
    // the addresses of the NEXT page to stage, read from the pointer table one tile ahead: a load behind the asm statements is a
    // vector load the compiler waits for with vmcnt(0) - asked for at the head of a tile it would stand in front of the tile's DMA
    int64_t pg_k = 0, pg_v = 0;
    auto fetch_table = [&](int p) {
        if (p < np) pg_k = ktab[p], pg_v = vtab[p];
    };
    auto load_page = [&](int p, int buf) {
        const uint8_t* kp = scalar_ptr(pg_k);             // (fetched one tile ahead: fetch_table)
        const uint8_t* vp = scalar_ptr(pg_v);
        const u32 fl = fresh_lane_id();                   // (not `lane`: nothing of this staging lives across the MFMA phases)
        const size_t doff = ((size_t)hkv * BN + 16 * wave) * DHB;
        const u32 lk = lds_k + buf * KS_BYTES + wave * 4096, lv = lds_v + buf * VT_BYTES + wave * 4096;
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            dma16(fl * (16 * NQ) + 16 * i, kp + doff, lk + 1024 * i);
            dma16(fl * (16 * NQ) + 16 * i, vp + doff, lv + 1024 * i);
        }
        // scales [Hkv][64] fp16 behind the data, then zeros [Hkv][64]
        const size_t moff = (size_t)num_kv_heads * BN * DHB + ((size_t)hkv * BN + 16 * wave) * 2;
        const u32 mo = ((fl >> 3) & 1u) * (u32)(num_kv_heads * BN * 2) + (fl & 7u) * 4u;
        dma4(mo, kp + moff, lk + RAW_META);
        dma4(mo, vp + moff, lv + RAW_META);
    };
    auto commit_page = [&](int p, int buf) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wave's own pieces are in LDS
        const int fl = (int)fresh_lane_id(), ptl = fl >> 2, pc4 = fl & 3;   // token within the wave's 16, quarter
        uint8_t* const wk = s_k + buf * KS_BYTES + wave * 4096;
        uint8_t* const wv = s_vt + buf * VT_BYTES + wave * 4096;
        v4u rk[NQ], rv[NQ];
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            rk[i] = *reinterpret_cast<const v4u*>(wk + 1024 * i + fl * 16);
            rv[i] = *reinterpret_cast<const v4u*>(wv + 1024 * i + fl * 16);
        }
        const int mofs = RAW_META + (ptl >> 1) * 4 + (ptl & 1) * 2;
        const _Float16 ks = *reinterpret_cast<const _Float16*>(wk + mofs), kz = *reinterpret_cast<const _Float16*>(wk + mofs + 32);
        const _Float16 vs = *reinterpret_cast<const _Float16*>(wv + mofs), vz = *reinterpret_cast<const _Float16*>(wv + mofs + 32);
        const int ptok = 16 * wave + ptl;
        const bool live = p * BN + ptok < past;          // slots >= past: anything may be there (NaN scales) - zeros, and masked
        const h8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
        h8 kd[4], vd[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) {                    // chunk 4 pc4 + m = dims 32 pc4 + 8 m .. + 7
            const u32 kw0 = INT4 ? rk[0][m] : rk[m >> 1][2 * (m & 1)], kw1 = INT4 ? 0u : rk[m >> 1][2 * (m & 1) + 1];
            const u32 vw0 = INT4 ? rv[0][m] : rv[m >> 1][2 * (m & 1)], vw1 = INT4 ? 0u : rv[m >> 1][2 * (m & 1) + 1];
            kd[m] = live ? dequant8<INT4>(kw0, kw1, ks, kz) : zero8;
            vd[m] = live ? dequant8<INT4>(vw0, vw1, vs, vz) : zero8;
        }
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int chunk = 4 * pc4 + m;
            *reinterpret_cast<h8*>(wk + ptl * 256 + ((chunk ^ (ptok & 15)) * 16)) = kd[m];
            *reinterpret_cast<h8*>(wv + ptl * 256 + ((chunk ^ ((ptok & 3) << 2)) * 16)) = vd[m];
        }
    };
    // tile t + 1 on its way while tile t is computed: a page's raw bytes (issue) that become its fp16 image behind the compute
    // (commit), or a tile of new keys straight into the other buffers
    auto issue_next = [&](int t, int nbuf) {
        if (t + 1 < np) load_page(t + 1, nbuf);
        else if (t + 1 < ntiles) load_new(t + 1 - np, nbuf);
    };
    auto commit_next = [&](int t, int nbuf) {
        if (t + 1 < np) commit_page(t + 1, nbuf);
        fetch_table(t + 2);                           // (lands under the wait for the tile)
    };

    v16f oacc[4];
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[d][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;

    fetch_table(0);
    issue_next(-1, 0);
    commit_next(-1, 0);
    // the Q fragments must be complete FOR THE COMPILER before the key loop (flash_prefill.hip: otherwise it waits for them, and with
    // them for the prefetch of the next tile, in front of the first MFMAs of every tile)
#pragma unroll
    for (int s = 0; s < 8; ++s) asm volatile("" : "+v"(qf[s]));
    tiles_landed();

    // rows of this wave: tokens tok_first .. tok_last (wave-uniform); a wave without a valid row only stages
    const int tok_first = tok0 + (wave * 32) / G;
    const int tok_last = tok0 + (wave * 32 + 31) / G;
    const bool wave_rows = wave * 32 < tq * G && tok_first < n;

    auto tile_body = [&](auto bufc, int t) {
        constexpr int buf = decltype(bufc)::value;
        issue_next(t, buf ^ 1);                       // lands in the other buffers during this tile

        v16f sacc[NKB];
        qk_tile(smem, bufc, lane, qf, sacc);
        h8 va[2][4];
        read_v(smem, bufc, lane, 0, va[0]);           // group 0 of the P.V operands, requested under the softmax
        __builtin_amdgcn_sched_barrier(0);
        // A page is masked where it holds slots >= past (its last one only), a tile of new keys where it touches the diagonal of a row
        // of this wave or the end of the new tokens (wave-uniform tests); `limit` = the last key of the tile this lane's row may see
        const bool page = t < np;
        const int j0 = (t - np) * BN;
        const bool need_mask = page ? t * BN + BN > past : j0 + BN - 1 > tok_first || j0 + BN > n;
        auto limit = [&] { return page ? past - 1 - t * BN : tok_ld - j0; };
        u32 pb[NKB][2][4];
        softmax_tile<true>(sacc, need_mask, limit, lane, scale_log2, m_run, l_run, oacc, pb);
        pv_tile(smem, bufc, lane, va, pb, oacc);
        commit_next(t, buf ^ 1);
        tiles_landed();
    };
    // tiles this WAVE computes: every page, and the tiles of new keys up to its last row's diagonal; for the rest it only takes part
    // in the staging and the barrier (a loop of its own: a skip path that rejoins the computing path inside the loop is a
    // control-flow merge the 64 O accumulators would be carried through - flash_prefill.hip)
    int nt_w = 0;
    if (wave_rows) {
        const int need = tok_last / BN + 1;
        nt_w = np + (need < nn ? need : nn);
    }
    // (two copies of the body, one per LDS buffer - every ds_read address a loop-invariant register + an immediate; an odd tile
    //  count leaves from the middle: a third copy behind the loop keeps its hoisted address registers alive across the loop)
    int t = 0;
    while (t < nt_w) {
        tile_body(std::integral_constant<int, 0>(), t);
        if (++t >= nt_w) break;
        tile_body(std::integral_constant<int, 1>(), t);
        ++t;
    }
    for (; t < ntiles; ++t) {
        issue_next(t, (t + 1) & 1);
        commit_next(t, (t + 1) & 1);
        tiles_landed();
    }
    if (!wave_rows) return;                              // (behind the last barrier)

    // ---- epilogue: normalise, fp16, out through LDS as whole 256-byte rows (store_rows_through_lds); row r of the workgroup goes
    // to (token tok0 + r / G, head hkv G + r % G)
    // (the two lines of the normaliser stay in the kernel: as a helper of flash_tile.h they cost this kernel ~50 registers and spills)
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    const float inv = l_tot > 0.f ? 1.0f / l_tot : 0.f;
    store_rows_through_lds(smem, wave, oacc, inv, [&](int rl, int cc, const v4u& x) {
        const int r = wave * 32 + rl;
        const int tok = tok0 + r / G;
        if (r < tq * G && tok < n)
            *reinterpret_cast<v4u*>(out + (size_t)(q_start + tok) * o_stride0 + (size_t)(hkv * G + r % G) * DH + cc * 8) = x;
    });
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
    const AppendPlan p = plan_append(max_seqlen_q, num_heads, num_kv_heads);
    plan3[0] = p.tile_tokens, plan3[1] = p.q_tiles, plan3[2] = p.waves;
    return QS_OK;
}

extern "C" int qs_append_attention(const void* qkv, void* out, const int32_t* cu_seqlens_q, const int32_t* past_lens,
                                   const int64_t* kv_pointers, int num_tokens, int batch, int max_seqlen_q, int max_blocks,
                                   int num_heads, int num_kv_heads, int head_dim, int64_t qkv_stride0, int64_t out_stride0,
                                   int tokens_per_block, int size_per_token, int int4_kv_cache, int kv_cache_with_zeros,
                                   qs_stream_t stream) {
    if (const int bad = check_append_args(qkv, out, cu_seqlens_q, past_lens, kv_pointers, num_tokens, batch, max_seqlen_q, max_blocks, num_heads,
                                          num_kv_heads, head_dim, qkv_stride0, out_stride0, tokens_per_block, size_per_token, int4_kv_cache,
                                          kv_cache_with_zeros); bad != QS_OK)
        return bad;
    int plan3[3];
    const int rc = qs_append_attention_plan(batch, max_seqlen_q, num_heads, num_kv_heads, plan3);
    if (rc != QS_OK) return rc;
    if (batch == 0 || max_seqlen_q == 0 || num_tokens == 0) return QS_OK;
    constexpr int SMEM = 2 * KS_BYTES + 2 * VT_BYTES;
    static bool lds_reserved[QS_MAX_DEVICES] = {};
    if (const hipError_t e = qs_reserve_lds({reinterpret_cast<const void*>(append_attention_kernel<true>), reinterpret_cast<const void*>(append_attention_kernel<false>)},
                                            SMEM, lds_reserved); e != hipSuccess) {
        qs_set_error("append_attention: cannot reserve %d bytes of LDS", SMEM);
        return (int)e;
    }
    const float scale_log2 = 0.08838834764831845f * 1.4426950408889634f;   // 1/sqrt(128) * log2(e)
    const dim3 grid(num_kv_heads, plan3[1], batch), block(64 * plan3[2]);
    if (int4_kv_cache)
        hipLaunchKernelGGL(append_attention_kernel<true>, grid, block, SMEM, (hipStream_t)stream, (const _Float16*)qkv, (_Float16*)out,
                           cu_seqlens_q, past_lens, kv_pointers, num_heads, num_kv_heads, max_blocks, plan3[0], qkv_stride0,
                           out_stride0, scale_log2);
    else
        hipLaunchKernelGGL(append_attention_kernel<false>, grid, block, SMEM, (hipStream_t)stream, (const _Float16*)qkv, (_Float16*)out,
                           cu_seqlens_q, past_lens, kv_pointers, num_heads, num_kv_heads, max_blocks, plan3[0], qkv_stride0,
                           out_stride0, scale_log2);
    return qs_launch_status("append_attention");
}
