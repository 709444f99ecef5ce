// append_walk.h -- what the append attention kernels share beyond the leaves of append_dequant.h: ONE walk of a workgroup over a range
// of a sequence's pages and, behind it, over the tile(s) of its new tokens, and the two ways a result leaves (normalised fp16 rows;
// the split-KV partial record).  Three translation units are built on it:
//   append_attention.hip        the whole past, causal new keys, normalised rows
//   append_attention_split.hip  a page range per workgroup, causal new keys behind the last range, partial records (+ the merge)
//   append_tree.hip             both of the above with the ANCESTOR MASK of tree-draft verification on the new keys
// A kernel decides WHO its rows are and WHICH key range it walks (sequence, KV head, query tile, split -> pages [p0, p0 + np), whether the
// new keys belong to it) and hands the walk a NEWKEYS policy - the mask of the new-key tiles, the only thing the tree kernels change:
//   int  count(n, tok0, tq)               new keys 0 .. count - 1 may be visible to some row of the query tile
//   int  tiles(tok_last, nn)              new-key tiles a wave whose last row is token tok_last has to compute (of nn)
//   bool needs_mask(j0, tok_first, n)     wave-uniform: the tile of new keys j0 .. j0 + 63 needs the mask
//   void mask(sacc, hi, page, page_limit, j0, tok_ld, n)   the (unlikely) mask block of a tile body, for this lane's row (token tok_ld): a
//                                         page (wave-uniform `page`) keeps its keys <= page_limit, a tile of new keys the policy's set  Everything is inlined into the kernel; the comments on the
// staging live here, once.
#pragma once
#include "append_dequant.h"
#include "attn_host.h"

namespace qs_append {

using namespace qs_flash;
using attn_plan::AppendPlan;
using attn_plan::MAX_SPLITS;
using attn_plan::REC_FLOATS;       // a wave's split-KV partial record (append_attention_split.hip has the layout)
static_assert(attn_plan::PAGE == BN && attn_plan::DH == DH && attn_plan::APPEND_WAVES == NWV && attn_plan::APPEND_ROWS == BM,
              "attn_plan.h plans for the tile geometry of flash_tile.h");

// The causal rule of append attention: new token i sees new keys 0 .. i.
struct CausalNewKeys {
    __device__ __forceinline__ int count(int n, int tok0, int tq) const { return n < tok0 + tq ? n : tok0 + tq; }
    __device__ __forceinline__ int tiles(int tok_last, int nn) const {      // up to its last row's diagonal
        const int need = tok_last / BN + 1;
        return need < nn ? need : nn;
    }
    // a tile of new keys is masked where it touches the diagonal of a row of this wave or the end of the new tokens
    __device__ __forceinline__ bool needs_mask(int j0, int tok_first, int n) const { return j0 + BN - 1 > tok_first || j0 + BN > n; }
    __device__ __forceinline__ void mask(v16f (&sacc)[NKB], int hi, bool page, int page_limit, int j0, int tok_ld, int n) const {
        mask_keys_above(sacc, page ? page_limit : tok_ld - j0, hi);
    }
};

// The walk.  Rows: row r = G * token + g of query tile tok0 .. tok0 + tq - 1 (wave w owns rows 32 w .. 32 w + 31); keys: pages
// ktab[0 .. np) / vtab[0 .. np) holding `past` cached tokens counted from ktab[0] (past >= np * BN: no slot masked), then - with_new -
// the n new tokens' fp16 k / v rows of KV head hkv in qkv.  Leaves the un-normalised O^T, the (lazy) running maximum and this lane
// half's sum; returns whether this wave has a row to store (false: it only staged; the caller returns - behind the last barrier).
template <bool INT4, class NEWKEYS>
__device__ __forceinline__ bool walk_keys(uint8_t* smem, const _Float16* __restrict__ qkv, const int64_t* __restrict__ ktab,
                                          const int64_t* __restrict__ vtab, int num_heads, int num_kv_heads, int hkv, int G, int q_start, int n,
                                          int tok0, int tq, int np, int past, bool with_new, int64_t qkv_stride0, float scale_log2,
                                          const NEWKEYS& newkeys, int lane, int wave, v16f (&oacc)[4], float& m_run, float& l_run) {
    constexpr int DHB = INT4 ? DH / 2 : DH;        // bytes per cached token and head
    constexpr int NQ = INT4 ? 1 : 2;               // 16-byte loads per thread, page and tensor
    uint8_t* const s_k = smem;                           // [2][16 KiB]  } the tile images of flash_tile.h
    uint8_t* const s_vt = smem + 2 * KS_BYTES;           // [2][16 KiB]  }
    const int nk_new = newkeys.count(n, tok0, tq);       // phase 2: new keys 0 .. nk_new - 1 are visible to some row
    const int nn = with_new ? (nk_new + BN - 1) / BN : 0;
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

#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[d][r] = 0.f;
    m_run = -INFINITY, l_run = 0.f;

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
        // A page is masked where it holds slots >= past (the sequence's last one only: key <= past - 1 - 64 t), a tile of new keys
        // where - and how - the policy says (wave-uniform tests)
        const bool page = t < np;
        const int j0 = (t - np) * BN;
        const bool need_mask = page ? t * BN + BN > past : newkeys.needs_mask(j0, tok_first, n);
        u32 pb[NKB][2][4];
        // (ONE block of 32 selects per tile body, whatever the tile is: a block per kind meets the other behind it, and the compiler
        //  carries copies of the 32 score registers to that merge - this kernel then spills)
        softmax_tile_masked<true>(sacc, need_mask, [&](v16f (&s)[NKB], int hi_) { newkeys.mask(s, hi_, page, past - 1 - t * BN, j0, tok_ld, n); },
                                  lane, scale_log2, m_run, l_run, oacc, pb);
        pv_tile(smem, bufc, lane, va, pb, oacc);
        commit_next(t, buf ^ 1);
        tiles_landed();
    };
    // tiles this WAVE computes: every page, and the tiles of new keys its rows can see; for the rest it only takes part in the
    // staging and the barrier (a loop of its own: a skip path that rejoins the computing path inside the loop is a control-flow
    // merge the 64 O accumulators would be carried through - flash_prefill.hip)
    int nt_w = 0;
    if (wave_rows) nt_w = np + newkeys.tiles(tok_last, nn);
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
    return wave_rows;
}

// ---- a result leaves, form 1: normalised, fp16, out through LDS as whole 256-byte rows (store_rows_through_lds); row r of the
// workgroup goes to (token tok0 + r / G, head hkv G + r % G).  A row that saw no key is exactly 0.
// (inv = 1 / (l_run + its other lane half's), or 0: the two lines of the normaliser stay in the kernels - inside a helper they cost
//  the un-split kernel ~50 registers and spills)
__device__ __forceinline__ void store_normalised_rows(uint8_t* smem, int wave, const v16f (&oacc)[4], float inv, _Float16* __restrict__ out,
                                                      int q_start, int n, int tok0, int tq, int G, int hkv, int64_t o_stride0) {
    store_rows_through_lds(smem, wave, oacc, inv, [&](int rl, int cc, const v4u& x) {
        const int r = wave * 32 + rl;
        const int tok = tok0 + r / G;
        if (r < tq * G && tok < n)
            *reinterpret_cast<v4u*>(out + (size_t)(q_start + tok) * o_stride0 + (size_t)(hkv * G + r % G) * DH + cc * 8) = x;
    });
}

// ---- form 2: the wave's split-KV partial record `rec` (REC_FLOATS floats), straight from the accumulator registers - lane
// (row li, half hi) holds dims 32 d + 8 rq + 4 hi .. + 3 of its row in oacc[d][4 rq ..], i.e. chunk 8 d + 2 rq + hi of the transposed
// record; no normalisation: O and l are relative to the (lazy) running maximum m, which goes with them.
__device__ __forceinline__ void store_partial_record(float* __restrict__ rec, const v16f (&oacc)[4], float m_run, float l_tot) {
    const int li_e = (int)(fresh_lane_id() & 31u), hi_e = (int)(fresh_lane_id() >> 5);
    float* const orow = rec + hi_e * 128 + li_e * 4;
    static_for<4>([&](auto dc) {
        constexpr int d = decltype(dc)::value;
        static_for<4>([&](auto rc) {
            constexpr int rq = decltype(rc)::value;
            const v4f o = {oacc[d][4 * rq], oacc[d][4 * rq + 1], oacc[d][4 * rq + 2], oacc[d][4 * rq + 3]};
            *reinterpret_cast<v4f*>(orow + (8 * d + 2 * rq) * 128) = o;
        });
    });
    if (hi_e == 0) {
        rec[32 * DH + li_e] = m_run;
        rec[32 * DH + 32 + li_e] = l_tot;
    }
}

// The page range of split `split` of `splits` over a past of past_all tokens (both split kernels and - as the test for a written
// record - the merge): pages [p0, p0 + np) of np_all = ceil(past_all / 64), ceil-sized, so the last range is the shortest.
struct PageRange {
    int p0, np;
};
__device__ __forceinline__ PageRange split_range(int past_all, int split, int splits) {
    const int np_all = (past_all + BN - 1) / BN;
    const int pps = (np_all + splits - 1) / splits;
    const int p0 = split * pps < np_all ? split * pps : np_all;
    return {p0, p0 + pps < np_all ? pps : np_all - p0};
}
__device__ __forceinline__ int clamp_past(int past, int max_blocks) {      // never walk beyond the pointer table
    return past < 0 ? 0 : past > max_blocks * BN ? max_blocks * BN : past;
}

// ---- the launch tail of every append attention kernel pair KERNEL<true> (KV4) / KERNEL<false> (KV8): the LDS reservation of the two
// K and two V tile images (once per pair and device: the flags belong to the pair, a reservation is never skipped because another
// kernel's was made), the softmax scale in log2 units - the kernels' LAST argument - and the choice of the instantiation.
// `entry` words the reservation's error, `what` the launch's.
template <auto KV4, auto KV8, class... Args>
int launch_kernel_pair(const char* entry, const char* what, bool int4, dim3 grid, dim3 block, hipStream_t stream, Args... args) {
    constexpr int SMEM = 2 * KS_BYTES + 2 * VT_BYTES;
    static bool lds_reserved[QS_MAX_DEVICES] = {};
    if (const hipError_t e = qs_reserve_lds({reinterpret_cast<const void*>(KV4), reinterpret_cast<const void*>(KV8)}, SMEM, lds_reserved);
        e != hipSuccess) {
        qs_set_error("%s: cannot reserve %d bytes of LDS", entry, SMEM);
        return (int)e;
    }
    const float scale_log2 = 0.08838834764831845f * 1.4426950408889634f;   // 1/sqrt(128) * log2(e)
    if (int4) hipLaunchKernelGGL(KV4, grid, block, SMEM, stream, args..., scale_log2);
    else hipLaunchKernelGGL(KV8, grid, block, SMEM, stream, args..., scale_log2);
    return qs_launch_status(what);
}

}  // namespace qs_append
