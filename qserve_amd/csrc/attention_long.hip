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
#include "append_dequant.h"
#include "attn_host.h"
#include "kv_quant.h"

namespace {

using attn_plan::LongPlan;
using qs_append::dequant8;
constexpr int PAGE_TOK = 64;
constexpr int DH = 128;
constexpr int NW = attn_plan::LONG_WAVES;
constexpr int TPB = NW * 64;
constexpr int DEPTH = 2;          // ring stages per wave
constexpr int WIN = 256;          // page addresses staged per window (K and V each)
constexpr int OS = DH + 4;        // row stride of the wave merge area
constexpr int NT_AUX = 2;         // non-temporal page DMA
static_assert(PAGE_TOK == attn_plan::PAGE && DH == attn_plan::DH && WIN % NW == 0 && NW == 4, "attn_plan.h plans for this file's geometry");

template <bool INT4>
struct Lds {
    static constexpr int DHB = INT4 ? DH / 2 : DH;           // bytes per token and head
    static constexpr int PAGE_BYTES = PAGE_TOK * DHB;
    static constexpr int NDMA = PAGE_BYTES / 1024;           // 1 KiB DMA instructions per page
    static constexpr int NVM = 2 * NDMA + 2;                 // VMEM instructions of one stage
    static constexpr int STAGE = 2 * PAGE_BYTES + 512;       // K | V | 4 x 64 halves
    static constexpr int RING = NW * DEPTH * STAGE;
    static constexpr int Q = RING;                           // fp16 [16][DH]
    static constexpr int WINDOW = Q + 16 * DH * 2;           // int64 [2][WIN]
    static constexpr int KNEW = WINDOW + 2 * WIN * 8;        // fp16 [DH]
    static constexpr int CUR = KNEW + DH * 2;                // float [16]
    static constexpr int ML = CUR + 64;                      // float [2][NW][16]
    static constexpr int BYTES = ML + 2 * NW * 16 * 4;
    static_assert(NW * 8 * OS * 4 <= RING, "the wave merge area must fit the rings");
};

typedef __attribute__((address_space(3))) const uint8_t* lds_u8;
#define LDS_AT(T, p) (*(const __attribute__((address_space(3))) T*)(p))
typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

// the quantiser of one (token, head) vector held two elements per lane by one wave (kv_quant.h: the decode kernels' bits)
template <bool INT4>
__device__ __forceinline__ void wave_quant_write(_Float16 v0, _Float16 v1, uint8_t* dst, __half* scale_p, __half* zero_p, int lane) {
    const float mx = wave_max(fmaxf((float)v0, (float)v1));
    const float mn = wave_min(fminf((float)v0, (float)v1));
    const QParams p = make_qparams<INT4>(mn, mx);
    const unsigned u0 = quant_u8(v0, p), u1 = quant_u8(v1, p);
    if (INT4) dst[lane] = (uint8_t)((u0 & 0xFu) | (u1 << 4));
    else *reinterpret_cast<uint16_t*>(dst + 2 * lane) = (uint16_t)(u0 | (u1 << 8));
    if (lane == 0) {
        *scale_p = __builtin_bit_cast(__half, p.scale);
        *zero_p = __builtin_bit_cast(__half, p.zero);
    }
}

template <bool INT4>
__global__ __launch_bounds__(TPB) void decode_long_kernel(
    const _Float16* __restrict__ q, const _Float16* __restrict__ k, const _Float16* __restrict__ v,
    const int64_t* __restrict__ kv_pointers, const int* __restrict__ lengths, _Float16* __restrict__ out, int num_heads,
    int num_kv_heads, int G, int64_t q_stride0, int64_t kv_stride0, int max_blocks, int timestep, float rope_base,
    const float2* __restrict__ rope_tab, int rope_tab_len, int S, int min_pages, float* __restrict__ ws) {
    using L = Lds<INT4>;
    constexpr int DHB = L::DHB, PAGE_BYTES = L::PAGE_BYTES;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    _Float16 (*s_q)[DH] = reinterpret_cast<_Float16 (*)[DH]>(smem + L::Q);
    int64_t (*s_win)[WIN] = reinterpret_cast<int64_t (*)[WIN]>(smem + L::WINDOW);
    _Float16* s_knew = reinterpret_cast<_Float16*>(smem + L::KNEW);
    float* s_cur = reinterpret_cast<float*>(smem + L::CUR);
    float (*s_m)[16] = reinterpret_cast<float (*)[16]>(smem + L::ML);
    float (*s_l)[16] = s_m + NW;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, tg = lane >> 4;
    const int hkv = blockIdx.x, b = blockIdx.y, z = blockIdx.z;
    const int tl = lengths ? lengths[b] - 1 : timestep;          // position of the new token = number of cached tokens
    float* const rec = ws ? ws + (((size_t)b * num_kv_heads + hkv) * S + z) * G * (DH + 2) : nullptr;

    // ---- this workgroup's range ----------------------------------------------------------------------------------------------
    const int npages = min((tl + PAGE_TOK - 1) >> 6, max_blocks);
    const int nr = max(1, min(S, npages / min_pages));
    if (tl < 0 || z >= nr) {                                     // nothing to read: the empty record (S > 1, or tl < 0)
        if (rec)
            for (int o = tid; o < G * (DH + 2); o += TPB) rec[o] = o % (DH + 2) == DH ? -3.0e38f : 0.f;
        return;
    }
    const int p_begin = z * npages / nr, p_end = (z + 1) * npages / nr;
    const bool writer = z == nr - 1;                             // the range that ends at the last page: the new token is its
    const int64_t* ktab = kv_pointers + (size_t)b * 2 * max_blocks;
    const int64_t* vtab = ktab + max_blocks;
    const float qk_scale = 0.08838834764831845f * 1.4426950408889634f;   // 1 / sqrt(128), scores in the log2 domain

    // ---- RoPE of the G query heads and of k; the writer quantises and stores the new token -------------------------------------
    const _Float16* qb = q + (size_t)b * q_stride0 + (size_t)hkv * G * DH;
    const _Float16* kb = k + (size_t)b * kv_stride0 + (size_t)hkv * DH;
    const _Float16* vb = v + (size_t)b * kv_stride0 + (size_t)hkv * DH;
    if (tid < 64) {
        RopeCS cs;
        if (rope_tab && tl < rope_tab_len) {
            const float2 t = rope_tab[(size_t)tl * 64 + tid];
            cs.c = t.x, cs.s = t.y;
        } else {
            cs = rope_coef_any(tid, tl, rope_base, DH, rope_tab);
        }
        for (int h = 0; h < G; ++h) {
            _Float16 a, bb;
            rope_pair((float)qb[h * DH + tid], (float)qb[h * DH + 64 + tid], cs, a, bb);
            s_q[h][tid] = a, s_q[h][64 + tid] = bb;
        }
        _Float16 a, bb;
        rope_pair((float)kb[tid], (float)kb[64 + tid], cs, a, bb);
        s_knew[tid] = a, s_knew[64 + tid] = bb;
    } else {
        for (int i = tid - 64; i < (16 - G) * DH; i += TPB - 64) s_q[G + i / DH][i % DH] = (_Float16)0.f;
    }
    __syncthreads();
    if (writer) {
        const int blk = tl >> 6, slot = tl & 63;
        if (wave < 2 && blk < max_blocks) {
            uint8_t* pg = reinterpret_cast<uint8_t*>(wave == 0 ? ktab[blk] : vtab[blk]);
            __half* sc = reinterpret_cast<__half*>(pg + (size_t)num_kv_heads * PAGE_BYTES);
            const _Float16 x0 = wave == 0 ? s_knew[2 * lane] : vb[2 * lane], x1 = wave == 0 ? s_knew[2 * lane + 1] : vb[2 * lane + 1];
            wave_quant_write<INT4>(x0, x1, pg + ((size_t)hkv * PAGE_TOK + slot) * DHB, sc + hkv * PAGE_TOK + slot,
                                   sc + (num_kv_heads + hkv) * PAGE_TOK + slot, lane);
        } else if (wave >= 2) {
            for (int h = wave - 2; h < G; h += NW - 2) {
                const float d = wave_sum((float)s_q[h][lane] * (float)s_knew[lane] + (float)s_q[h][64 + lane] * (float)s_knew[64 + lane]);
                if (lane == 0) s_cur[h] = d * qk_scale;
            }
        }
    }
    // B operand of Q.K^T for the whole walk: head li, dims 32 tg + 8 w .. + 7
    h8 qB[4];
#pragma unroll
    for (int w = 0; w < 4; ++w) qB[w] = *reinterpret_cast<const h8*>(&s_q[li][32 * tg + 8 * w]);

    v4f acc[8];                      // acc[e][r]: out dim 8 (4 tg + r) + e of head li
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = (v4f){0.f, 0.f, 0.f, 0.f};
    float m_run = -3.0e38f, l_part = 0.f;

    uint8_t* const ring = smem + wave * (DEPTH * L::STAGE);
    for (int wbase = p_begin; wbase < p_end; wbase += WIN) {
        const int wend = min(wbase + WIN, p_end);
        __syncthreads();                                         // the window before is consumed (first pass: s_cur, s_q are written)
        if (tid < wend - wbase) {
            s_win[0][tid] = ktab[wbase + tid];
            s_win[1][tid] = vtab[wbase + tid];
        }
        __syncthreads();
        // one stage: K page, k scales | zeros, V page, v scales | zeros
        auto issue = [&](int p, int st) {
            uint8_t* const stage = ring + st * L::STAGE;
            const uint8_t* kpage = reinterpret_cast<const uint8_t*>(s_win[0][p - wbase]);
            const uint8_t* vpage = reinterpret_cast<const uint8_t*>(s_win[1][p - wbase]);
            const u32 meta = (u32)(num_kv_heads * PAGE_BYTES + ((lane >> 5) * num_kv_heads + hkv) * (PAGE_TOK * 2) + (lane & 31) * 4);
            const uint8_t* kd = kpage + (u32)(hkv * PAGE_BYTES);
            const uint8_t* vd = vpage + (u32)(hkv * PAGE_BYTES);
#pragma unroll
            for (int e = 0; e < L::NDMA; ++e) {
                u32 off;
                if (INT4) {
                    off = e * 1024 + lane * 16;
                } else {
                    const int row = 8 * e + (lane >> 3);
                    off = row * DHB + (((lane & 7) ^ ((row >> 1) & 7)) * 16);
                }
                __builtin_amdgcn_global_load_lds((gptr_t)(kd + off), (lptr_t)(stage + e * 1024), 16, 0, NT_AUX);
            }
            __builtin_amdgcn_global_load_lds((gptr_t)(kpage + meta), (lptr_t)(stage + 2 * PAGE_BYTES), 4, 0, 0);
#pragma unroll
            for (int e = 0; e < L::NDMA; ++e) {
                constexpr int CPR = DHB / 16;                    // 16-byte chunks per token row
                const int slot = (64 / L::NDMA) * e + lane / CPR;
                const int tok = (slot & ~3) | ((slot - (slot >> 2)) & 3);
                const u32 off = tok * DHB + (lane % CPR) * 16;
                __builtin_amdgcn_global_load_lds((gptr_t)(vd + off), (lptr_t)(stage + PAGE_BYTES + e * 1024), 16, 0, NT_AUX);
            }
            __builtin_amdgcn_global_load_lds((gptr_t)(vpage + meta), (lptr_t)(stage + 2 * PAGE_BYTES + 256), 4, 0, 0);
        };
        int p = wbase + wave;
        if (p < wend) issue(p, 0);
        if (p + NW < wend) issue(p + NW, 1);
        for (int st = 0; p < wend; p += NW, st ^= 1) {
            // page p landed?  Younger VMEM instructions at this point: the NVM of page p + NW, where there is one.
            if (p + NW < wend) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(L::NVM) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const int valid = min(PAGE_TOK, tl - p * PAGE_TOK);
            const lds_u8 kl = (lds_u8)(ring + st * L::STAGE), vl = kl + PAGE_BYTES, ml = kl + 2 * PAGE_BYTES;

            // ---------------- Q.K^T: 4 tiles of 16 tokens; sc[t][r] = token 16 t + 4 tg + r, head li ----------------
            float sc[4][4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int row = 16 * t + li;
                const _Float16 ks = LDS_AT(_Float16, ml + 2 * row), kz = LDS_AT(_Float16, ml + 128 + 2 * row);
                v4f c = {0.f, 0.f, 0.f, 0.f};
                if (INT4) {
                    const v4u raw = LDS_AT(v4u, kl + row * DHB + tg * 16);
#pragma unroll
                    for (int w = 0; w < 4; ++w) c = __builtin_amdgcn_mfma_f32_16x16x32_f16(dequant8<true>(raw[w], 0, ks, kz), qB[w], c, 0, 0, 0);
                } else {
                    const int sw = (row >> 1) & 7;
                    const v4u ra = LDS_AT(v4u, kl + row * DHB + (((2 * tg) ^ sw) * 16));
                    const v4u rb = LDS_AT(v4u, kl + row * DHB + (((2 * tg + 1) ^ sw) * 16));
                    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(dequant8<false>(ra[0], ra[1], ks, kz), qB[0], c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(dequant8<false>(ra[2], ra[3], ks, kz), qB[1], c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(dequant8<false>(rb[0], rb[1], ks, kz), qB[2], c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(dequant8<false>(rb[2], rb[3], ks, kz), qB[3], c, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float s = c[r];
                    sc[t][r] = 16 * t + 4 * tg + r < valid ? s * qk_scale : -3.0e38f;      // (a select: unwritten slots may hold NaN)
                }
            }
            // ---------------- online softmax of head li over the page (its 64 scores sit in the 4 lanes li + 16 tg) ----------------
            float mx = sc[0][0];
#pragma unroll
            for (int j = 1; j < 16; ++j) mx = fmaxf(mx, sc[j >> 2][j & 3]);
            mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float m_new = fmaxf(m_run, mx);
            const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
            m_run = m_new;
            l_part *= alpha;
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] *= alpha;
            u32 pk[4][2];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                float pe[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    pe[r] = __builtin_amdgcn_exp2f(sc[t][r] - m_new);   // 0 for masked tokens
                    l_part += pe[r];
                }
                pk[t][0] = pack_h2(pe[0], pe[1]), pk[t][1] = pack_h2(pe[2], pe[3]);
            }
            // ---------------- P.V: two half pages; the lane's 8 tokens of half hp are 32 hp + 16 jh + 4 tg + r ----------------
#pragma unroll
            for (int hp = 0; hp < 2; ++hp) {
                const h8 pB = __builtin_bit_cast(h8, (v4u){pk[2 * hp][0], pk[2 * hp][1], pk[2 * hp + 1][0], pk[2 * hp + 1][1]});
                h8 d[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int r = j & 3, tok = 32 * hp + 16 * (j >> 2) + 4 * tg + r;
                    const int slot = 32 * hp + 16 * (j >> 2) + 4 * tg + ((r + tg) & 3);
                    _Float16 vs = LDS_AT(_Float16, ml + 256 + 2 * tok), vz = LDS_AT(_Float16, ml + 384 + 2 * tok);
                    if (tok >= valid) vs = (_Float16)0.f, vz = (_Float16)0.f;      // unwritten slots de-quantise to 0, not to NaN
                    if (INT4) {
                        d[j] = dequant8<true>(LDS_AT(u32, vl + slot * DHB + 4 * li), 0, vs, vz);
                    } else {
                        const v2u raw = LDS_AT(v2u, vl + slot * DHB + 8 * li);
                        d[j] = dequant8<false>(raw.x, raw.y, vs, vz);
                    }
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const h8 a_e = {d[0][e], d[1][e], d[2][e], d[3][e], d[4][e], d[5][e], d[6][e], d[7][e]};
                    acc[e] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_e, pB, acc[e], 0, 0, 0);
                }
            }
            // the stage is consumed: page p + 2 NW takes it
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (p + 2 * NW < wend) issue(p + 2 * NW, st);
        }
    }

    // ---- waves -> LDS (the dead rings), then one result per head: `out`, or the range's record -------------------------------------
    l_part += __shfl_xor(l_part, 16, 64);
    l_part += __shfl_xor(l_part, 32, 64);
    __syncthreads();                                             // every wave has drained its ring (and passed the prologue)
    float (*s_o)[8][OS] = reinterpret_cast<float (*)[8][OS]>(smem);
    if (li < G) {
#pragma unroll
        for (int e = 0; e < 8; ++e)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float x = acc[e][r];
                s_o[wave][li][8 * (4 * tg + r) + e] = x;
            }
        if (tg == 0) s_m[wave][li] = m_run, s_l[wave][li] = l_part;
    }
    __syncthreads();
    for (int o = tid; o < G * DH; o += TPB) {
        const int h = o / DH, d = o % DH;
        float M = writer ? s_cur[h] : -3.0e38f;
#pragma unroll
        for (int w = 0; w < NW; ++w) M = fmaxf(M, s_m[w][h]);
        const float pc = writer ? __builtin_amdgcn_exp2f(s_cur[h] - M) : 0.f;      // the new token's own term
        float num = pc * (float)vb[d], den = pc;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const float f = __builtin_amdgcn_exp2f(s_m[w][h] - M);
            num += f * s_o[w][h][d];
            den += f * s_l[w][h];
        }
        if (!rec) {
            out[((size_t)b * num_heads + (size_t)hkv * G + h) * DH + d] = (_Float16)(num / (den + 1.e-6f));
        } else {                                                 // un-normalised: [O(128) | m | l], m in natural-log units (the merge's)
            float* pw = rec + h * (DH + 2);
            pw[d] = num;
            if (d == 0) pw[DH] = M * 0.6931471805599453f, pw[DH + 1] = den;
        }
    }
}

int single_query_attention_long(const void* q, const void* k, const void* v, const int64_t* kv_pointers, const int32_t* length_per_sample,
                                void* out, int batch, int num_heads, int num_kv_heads, int head_dim, int64_t q_stride0, int64_t kv_stride0,
                                int max_blocks, int memory_max_seqlen, int tokens_per_block, int size_per_token, int timestep,
                                int rotary_embedding_dim, float rotary_base, int int4_kv_cache, int kv_cache_with_zeros, int num_splits,
                                qs_stream_t stream) {
    QS_REQUIRE(q && k && v && kv_pointers && out, "single_query_attention_long: null pointer");
    QS_REQUIRE(batch >= 0 && num_heads > 0 && num_kv_heads > 0 && num_heads % num_kv_heads == 0,
               "single_query_attention_long: bad head counts H=%d Hkv=%d", num_heads, num_kv_heads);
    const int G = num_heads / num_kv_heads;
    if (head_dim != 128 || rotary_embedding_dim != 128 || tokens_per_block != 64 || !kv_cache_with_zeros || G > 8) {
        qs_set_error("single_query_attention_long: only head_dim=128, rotary_dim=128, tokens_per_block=64, zero-point KV caches and "
                     "num_heads/num_kv_heads in 1..8 are supported (H=%d Hkv=%d)", num_heads, num_kv_heads);
        return QS_ENOSUP;
    }
    const int dhb = int4_kv_cache ? 64 : 128;
    QS_REQUIRE(size_per_token == num_kv_heads * dhb, "single_query_attention_long: size_per_token=%d, expected %d", size_per_token,
               num_kv_heads * dhb);
    QS_REQUIRE(max_blocks > 0 && memory_max_seqlen > 0, "single_query_attention_long: bad max_blocks / memory_max_seqlen");
    QS_REQUIRE(num_splits >= 0, "single_query_attention_long: num_splits=%d (0 = choose, >= 1 = that many ranges)", num_splits);
    QS_REQUIRE(q_stride0 % 8 == 0 && kv_stride0 % 8 == 0 && q_stride0 >= (int64_t)num_heads * 128 && kv_stride0 >= (int64_t)num_kv_heads * 128,
               "single_query_attention_long: token strides must hold the token's heads and keep 16-byte alignment");
    QS_REQUIRE(((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(v) |
                 reinterpret_cast<uintptr_t>(out)) & 15) == 0,
               "single_query_attention_long: q, k, v and out must be 16-byte aligned");
    QS_REQUIRE(batch <= 65535 && num_kv_heads <= 65535, "single_query_attention_long: batch and num_kv_heads are grid dimensions (<= 65535)");
    if (batch == 0) return QS_OK;
    LongPlan plan = attn_plan::plan_decode_long(batch, num_kv_heads, G, max_blocks, int4_kv_cache != 0, qs_split_workspace_capacity());
    if (num_splits >= 1) plan.splits = num_splits > attn_plan::MAX_SPLITS ? attn_plan::MAX_SPLITS : num_splits;
    DecodeLongArgs a;
    a.int4 = int4_kv_cache != 0, a.batch = batch;
    DecodeArgs& d = a.d;
    d.G = G, d.grid = dim3(num_kv_heads, batch), d.st = (hipStream_t)stream;
    d.q = (const _Float16*)q, d.k = (const _Float16*)k, d.v = (const _Float16*)v, d.kvp = kv_pointers, d.len = length_per_sample;
    d.out = (_Float16*)out, d.H = num_heads, d.Hkv = num_kv_heads, d.qs = q_stride0, d.kvs = kv_stride0, d.mb = max_blocks;
    d.timestep = timestep, d.base = rotary_base, d.max_pos = memory_max_seqlen, d.quant = nullptr, d.fused = nullptr;
    return qs_launch_decode_long(a, plan);
}

}  // namespace

int qs_launch_decode_long(const DecodeLongArgs& a, const LongPlan& plan) {
    QS_DECODE_LOCALS(a.d);
    int tab_len = 0;
    const float2* tab = qs_rope_table(base, max_pos, st, &tab_len);
    if (base < 0.f && !tab) return QS_EINVAL;      // a profile key that is not registered on this device (qs_last_error says which)
    const size_t per_split = attn_plan::decode_split_bytes(Hkv * a.batch, G);
    int S = plan.splits > 1 ? attn_plan::fit_splits(plan.splits, per_split, qs_split_workspace_capacity(), attn_plan::MAX_SPLITS) : 1;
    float* ws = S > 1 ? qs_split_workspace(per_split * S, st) : nullptr;
    if (!ws) S = 1;                                // beyond the capacity, or its first use inside a capture: one range, `out` directly
    grid.z = S;
    static bool lds4[QS_MAX_DEVICES] = {}, lds8[QS_MAX_DEVICES] = {};
    const int bytes = a.int4 ? Lds<true>::BYTES : Lds<false>::BYTES;
    const void* kern = a.int4 ? reinterpret_cast<const void*>(decode_long_kernel<true>) : reinterpret_cast<const void*>(decode_long_kernel<false>);
    if (const hipError_t e = qs_reserve_lds({kern}, bytes, a.int4 ? lds4 : lds8); e != hipSuccess) {
        qs_set_error("single_query_attention_long: cannot reserve %d bytes of LDS: %s", bytes, hipGetErrorString(e));
        return (int)e;
    }
    if (a.int4)
        hipLaunchKernelGGL(decode_long_kernel<true>, grid, dim3(TPB), bytes, st, q, k, v, kvp, len, out, H, Hkv, G, qs, kvs, mb, timestep, base,
                           tab, tab_len, S, plan.min_pages, ws);
    else
        hipLaunchKernelGGL(decode_long_kernel<false>, grid, dim3(TPB), bytes, st, q, k, v, kvp, len, out, H, Hkv, G, qs, kvs, mb, timestep, base,
                           tab, tab_len, S, plan.min_pages, ws);
    if (S > 1) qs_launch_attention_merge(ws, out, H, Hkv, G, S, a.batch, st);
    return qs_launch_status("single_query_attention_long");
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
