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
#include "append_dequant.h"

float* qs_split_workspace(size_t bytes, hipStream_t st);     // attention_mfma.hip
size_t qs_split_workspace_capacity();

namespace {

using namespace qs_flash;
using namespace qs_append;

constexpr int REC_FLOATS = 32 * (DH + 2);          // one wave's block: O^T [32 chunks][32 rows][4], m[32], l[32]
constexpr int MAX_SPLITS = 64;

// ---- the planner's rule (pure; qs_append_attention_split_plan) -------------------------------------------------------------
// "Fill the CUs once" (the decode chooser's form): the un-split grid has base = batch * Hkv * q_tiles workgroups and the
// chip holds FILL of them at a time (256 CUs x two 64 KiB workgroups); below that, split until the chip is full, but never below
// MIN_PAGES pages per split (a split pays its own Q load, pipeline fill, 65 KiB of partial records and its share of the merge) and
// never for a past of fewer than 128 tokens.
// Fitted to scripts/bench_append_split.py -> profiles/append_split.txt (MI355X, Llama-3-8B heads):
//   FILL = 512       B = 8, past 4096, n = 4 (base 64): 4 splits 44 us, 7 splits (what the workspace holds of 512 / 64 = 8) 40 us -
//                    filling both workgroup slots of every CU still pays; no correction to the starting form.
//   MIN_PAGES = 8    B = 1, past 8192, n = 8: 16 splits (8 pages each) 33.6 us KV4 / 35.1 us KV8, 32 splits (4 pages each) 34.0 /
//                    37.8 us - below 8 pages per split the merge and the per-split set-up cost what the shorter chain saves.
//                    At short pasts it is too high (B = 1, n = 8, past 1024: 2 splits 25.9 us, 8 splits 18.0 us; past 2048: 4 splits
//                    26.8 us, 8 splits 21.6 us - still ahead of un-split, 37.0 / 65.2 us): the regret is in the profile and DESIGN 10.
constexpr int FILL = 512;
constexpr int MIN_PAGES = 8;
int plan_splits(int batch, int q_tiles, int num_kv_heads, int max_past) {
    const long base = (long)batch * num_kv_heads * q_tiles;
    if (base <= 0 || base >= FILL || max_past < 2 * BN) return 1;
    const int pages = (max_past + BN - 1) / BN;
    long s = FILL / base;
    if (s > pages / MIN_PAGES) s = pages / MIN_PAGES;
    const long cap = (long)(qs_split_workspace_capacity() / ((size_t)base * NWV * REC_FLOATS * sizeof(float)));
    if (s > cap) s = cap;
    if (s > MAX_SPLITS) s = MAX_SPLITS;
    return s < 1 ? 1 : (int)s;
}

template <bool INT4>
__global__ __launch_bounds__(64 * NWV, 2) void append_attention_split_kernel(const _Float16* __restrict__ qkv, float* __restrict__ ws,
                                                                            const int* __restrict__ cu_q, const int* __restrict__ past_lens,
                                                                            const int64_t* __restrict__ kv_pointers, int num_heads,
                                                                            int num_kv_heads, int max_blocks, int tq, int q_tiles, int splits,
                                                                            int64_t qkv_stride0, float scale_log2) {
    constexpr int DHB = INT4 ? DH / 2 : DH;        // bytes per cached token and head
    constexpr int NQ = INT4 ? 1 : 2;               // 16-byte loads per thread, page and tensor
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint8_t* const s_k = smem;                           // [2][16 KiB]  } the tile images of flash_tile.h
    uint8_t* const s_vt = smem + 2 * KS_BYTES;           // [2][16 KiB]  }

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // grid = (KV heads, query tiles x splits, sequences); the splits of a query tile are neighbours, the tiles run last-to-first
    const int hkv = blockIdx.x, b = blockIdx.z;
    const int split = (int)blockIdx.y % splits, qt = q_tiles - 1 - (int)blockIdx.y / splits;
    const int G = num_heads / num_kv_heads;
    const int q_start = cu_q[b], n = cu_q[b + 1] - q_start;
    const int tok0 = qt * tq;                            // first new token of this tile
    if (tok0 >= n) return;                               // (n = 0: nothing read, nothing written)
    int past_all = past_lens[b];
    past_all = past_all < 0 ? 0 : past_all > max_blocks * BN ? max_blocks * BN : past_all;   // never walk beyond the pointer table
    // this split's pages [p0, p0 + np) of the sequence's np_all; `past` = the cached tokens counted from page p0 (beyond np * BN for
    // every range but the one that holds the last page: no slot of those ranges is masked)
    const int np_all = (past_all + BN - 1) / BN;
    const int pps = (np_all + splits - 1) / splits;
    const int p0 = split * pps < np_all ? split * pps : np_all;
    const int np = p0 + pps < np_all ? pps : np_all - p0;
    const bool with_new = split == splits - 1;           // the last split also serves phase 2
    if (np == 0 && !with_new) return;                    // EMPTY: no record (the merge recomputes this test)
    const int past = past_all - p0 * BN;
    const int nk_new = n < tok0 + tq ? n : tok0 + tq;    // phase 2: new keys 0 .. nk_new - 1 are visible to some row
    const int nn = with_new ? (nk_new + BN - 1) / BN : 0;
    const int ntiles = np + nn;

    const int li = lane & 31, hi = lane >> 5;
    const int r_w = wave * 32 + li;                      // this lane's row (both lane halves share it)
    const int tok_r = tok0 + r_w / G;                    // its token; rows >= tq * G and tokens >= n compute, but are never merged
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

    // ---- phase 1 staging, as in append_attention.hip (the comments there): wave w drops the raw bytes of tokens 16w .. 16w+15 of a
    // page into the tile rows they become, and de-quantises them in place behind the P.V products.  Page p of this split is entry
    // p0 + p of the sequence's pointer table.
    const int64_t* ktab = kv_pointers + (size_t)b * 2 * max_blocks + p0;
    const int64_t* vtab = ktab + max_blocks;
    constexpr int RAW_META = 2048;                       // raw data at + 0 (1 KiB KV4 / 2 KiB KV8), the parameters behind it
    auto dma4 = [&](u32 voff, const void* sbase, u32 lds_addr) {
        asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %0, %1" ::"v"(voff), "s"(sbase), "s"(lds_addr) : "memory");
    };
    int64_t pg_k = 0, pg_v = 0;                          // the NEXT page's addresses, read from the table one tile ahead
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
    // the Q fragments must be complete FOR THE COMPILER before the key loop (flash_prefill.hip)
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
        // A page is masked where it holds slots >= past (the sequence's last one only), a tile of new keys where it touches the
        // diagonal of a row of this wave or the end of the new tokens (wave-uniform tests)
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
    // tiles this WAVE computes: every page of the split, and the tiles of new keys up to its last row's diagonal (append_attention.hip)
    int nt_w = 0;
    if (wave_rows) {
        const int need = tok_last / BN + 1;
        nt_w = np + (need < nn ? need : nn);
    }
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
    if (!wave_rows) return;                              // (behind the last barrier; the merge skips this wave's block by the same test)

    // ---- epilogue: the wave's partial record, straight from the accumulator registers (layout: the head of this file)
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    const size_t wg = ((size_t)b * q_tiles + qt) * num_kv_heads + hkv;
    float* const rec = ws + ((wg * splits + split) * NWV + wave) * REC_FLOATS;
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

extern "C" int qs_append_attention_split_plan(int batch, int max_seqlen_q, int max_past, int num_heads, int num_kv_heads,
                                              int int4_kv_cache, int* plan5) {
    QS_REQUIRE(plan5, "append attention split plan: null output");
    plan5[0] = plan5[1] = plan5[2] = plan5[3] = plan5[4] = 0;
    QS_REQUIRE(max_past >= 0, "append_attention_split: negative max_past");
    const int rc = qs_append_attention_plan(batch, max_seqlen_q, num_heads, num_kv_heads, plan5);   // (checks the rest, fills 0 .. 2)
    if (rc != QS_OK || plan5[1] == 0) return rc;
    (void)int4_kv_cache;                                 // both cache types walk 64-token pages: one rule
    const int splits = plan_splits(batch, plan5[1], num_kv_heads, max_past);
    plan5[3] = splits;
    // KiB of partial records (a record block is 16 640 B, four per workgroup: 65 KiB); 0 for the un-split launch, which has none
    plan5[4] = splits > 1 ? (int)((size_t)batch * num_kv_heads * plan5[1] * splits * (NWV * REC_FLOATS * sizeof(float) / 1024)) : 0;
    return QS_OK;
}

extern "C" int qs_append_attention_split(const void* qkv, void* out, const int32_t* cu_seqlens_q, const int32_t* past_lens,
                                         const int64_t* kv_pointers, int num_tokens, int batch, int max_seqlen_q, int max_blocks,
                                         int num_heads, int num_kv_heads, int head_dim, int64_t qkv_stride0, int64_t out_stride0,
                                         int tokens_per_block, int size_per_token, int int4_kv_cache, int kv_cache_with_zeros,
                                         int max_past, int num_splits, qs_stream_t stream) {
    if (const int bad = check_append_args(qkv, out, cu_seqlens_q, past_lens, kv_pointers, num_tokens, batch, max_seqlen_q, max_blocks, num_heads,
                                          num_kv_heads, head_dim, qkv_stride0, out_stride0, tokens_per_block, size_per_token, int4_kv_cache,
                                          kv_cache_with_zeros); bad != QS_OK)
        return bad;
    QS_REQUIRE(num_splits >= 0, "append_attention_split: num_splits=%d (0 = ask the planner, >= 1 = forced)", num_splits);
    int plan5[5];
    const int hint = max_past < 0 || max_past > max_blocks * BN ? max_blocks * BN : max_past;   // (a past is cut to the table anyway)
    const int rc = qs_append_attention_split_plan(batch, max_seqlen_q, hint, num_heads, num_kv_heads, int4_kv_cache, plan5);
    if (rc != QS_OK) return rc;
    if (batch == 0 || max_seqlen_q == 0 || num_tokens == 0) return QS_OK;
    // the effective split count: the planner's or the forced one, at most 64 and what the workspace holds
    int splits = num_splits > 0 ? num_splits : plan5[3];
    const size_t per_split = (size_t)batch * num_kv_heads * plan5[1] * NWV * REC_FLOATS * sizeof(float);
    if (splits > MAX_SPLITS) splits = MAX_SPLITS;
    if (per_split * splits > qs_split_workspace_capacity()) splits = (int)(qs_split_workspace_capacity() / per_split);
    float* const ws = splits > 1 ? qs_split_workspace(per_split * splits, (hipStream_t)stream) : nullptr;
    if (!ws)      // one split, or no workspace (first use inside a capture): the un-split launch, bit for bit qs_append_attention
        return qs_append_attention(qkv, out, cu_seqlens_q, past_lens, kv_pointers, num_tokens, batch, max_seqlen_q, max_blocks, num_heads,
                                   num_kv_heads, head_dim, qkv_stride0, out_stride0, tokens_per_block, size_per_token, int4_kv_cache,
                                   kv_cache_with_zeros, stream);
    constexpr int SMEM = 2 * KS_BYTES + 2 * VT_BYTES;
    static bool lds_reserved[QS_MAX_DEVICES] = {};
    if (const hipError_t e = qs_reserve_lds({reinterpret_cast<const void*>(append_attention_split_kernel<true>),
                                             reinterpret_cast<const void*>(append_attention_split_kernel<false>)},
                                            SMEM, lds_reserved); e != hipSuccess) {
        qs_set_error("append_attention_split: cannot reserve %d bytes of LDS", SMEM);
        return (int)e;
    }
    const float scale_log2 = 0.08838834764831845f * 1.4426950408889634f;   // 1/sqrt(128) * log2(e)
    const int tq = plan5[0], q_tiles = plan5[1];
    const dim3 grid(num_kv_heads, q_tiles * splits, batch), block(64 * plan5[2]);
    if (int4_kv_cache)
        hipLaunchKernelGGL(append_attention_split_kernel<true>, grid, block, SMEM, (hipStream_t)stream, (const _Float16*)qkv, ws, cu_seqlens_q,
                           past_lens, kv_pointers, num_heads, num_kv_heads, max_blocks, tq, q_tiles, splits, qkv_stride0, scale_log2);
    else
        hipLaunchKernelGGL(append_attention_split_kernel<false>, grid, block, SMEM, (hipStream_t)stream, (const _Float16*)qkv, ws, cu_seqlens_q,
                           past_lens, kv_pointers, num_heads, num_kv_heads, max_blocks, tq, q_tiles, splits, qkv_stride0, scale_log2);
    if (const int lrc = qs_launch_status("append_attention_split"); lrc != QS_OK) return lrc;
    hipLaunchKernelGGL(append_attention_merge_kernel, dim3(num_kv_heads, q_tiles * NWV, batch), dim3(256), 0, (hipStream_t)stream, ws,
                       (_Float16*)out, cu_seqlens_q, past_lens, num_heads, num_kv_heads, max_blocks, tq, q_tiles, splits, out_stride0);
    return qs_launch_status("append_attention_merge");
}
