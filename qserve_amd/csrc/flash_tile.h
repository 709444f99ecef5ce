// flash_tile.h -- the flash-attention tile core of MI355X (gfx950), once: what a 4-wave workgroup does with ONE 64-key tile of fp16
// K / V rows in LDS, as device functions behind the kernels that walk key tiles - the prefill provider (flash_prefill.hip) and
// append attention over the quantised KV cache (append_walk.h: append_attention.hip, append_attention_split.hip, append_tree.hip).  The two differ in WHO the 128 rows of a workgroup are and
// WHERE a tile comes from (their key range, tile schedule, page staging and row mapping stay in their own files); the tile itself -
// its LDS images, the two swapped MFMA products, the online softmax between them and the way O leaves - is this header:
//   * workgroup = 4 wave64 = 128 rows; wave w owns 32 rows and keeps their Q fragments (8 x 16 dims) in registers;
//   * key/value tiles of 64 keys are staged through LDS once per workgroup (shared by the 4 waves): K row-major with a 16-byte XOR
//     swizzle, V row-major too (16-byte chunk ^ 4 (key & 3): the 32 lanes of a transpose read then hit 32 distinct 8-byte slots;
//     chunk ^ 2 (key & 3), the round-1 form, left them two-way conflicted - SQ_LDS_BANK_CONFLICT was a third of the LDS cycles) and
//     TRANSPOSED ON READ by ds_read_b64_tr_b16, both tiles double-buffered, one barrier per tile;
//   * "swapped" products on v_mfma_f32_32x32x16_f16:  S^T = K Q^T  (A = K rows, B = Q rows, both plain 16-byte reads)
//     leaves every lane holding 16 of the 32 scores of ITS OWN query row, so the softmax is register-only (one
//     cross-lane max with lane ^ 32) and the probabilities already sit in B-operand order for
//     O^T = V^T P^T  (A = V^T fragments, two transpose reads each; k-slot <-> key mapping chosen to match the S^T layout);
//   * exp2 with the scale folded into one fp32 multiply; rescaling of O only through the running max.
// Every function is inlined into the caller's key loop; the LDS buffer index `bufc` is a std::integral_constant where the caller's
// loop is unrolled over the two buffers (every ds_read address a loop-invariant register + an immediate offset) or a run-time int.
// `lane` is the caller's threadIdx.x & 63: lane (li = lane & 31, hi = lane >> 5) holds row li of its wave, both halves share it.
#pragma once
#include "common.h"

namespace qs_flash {

typedef float v16f __attribute__((ext_vector_type(16)));

constexpr int DH = 128;
constexpr int NWV = 4;            // waves per workgroup (32 rows each)
constexpr int BM = 32 * NWV;      // rows per workgroup
constexpr int PPW = 16 / NWV;     // 1 KiB DMA pieces of a K (and of a V) tile per wave
constexpr int NKB = 2;            // 32-key blocks per tile
constexpr int BN = 32 * NKB;      // keys per tile (= tokens per KV page)
constexpr int KS_BYTES = BN * DH * 2;             // 16 KiB
constexpr int VT_BYTES = BN * DH * 2;             // 16 KiB (row-major like K; transposed on read)
constexpr int OST = 272;                          // row stride of the epilogue's O staging (store_rows_through_lds)
static_assert(BN == 64, "the DMA staging is written for 64-key tiles");
static_assert(PPW == 4 && PPW * NWV * 1024 == KS_BYTES, "the per-piece offsets are derived for four 1 KiB pieces per wave");
static_assert(NWV * 32 * OST <= 2 * KS_BYTES + 2 * VT_BYTES, "the epilogue stages every wave's 32 output rows inside the (dead) tile buffers");

__device__ __forceinline__ u32 lds_address(const void* p) {
    typedef __attribute__((address_space(3))) void* lptr_t;
    return (u32)(size_t)(lptr_t)p;
}

// ---- tile staging by LDS-DMA: a 1 KiB piece = 4 keys x 256 B; wave w copies K pieces 4w .. 4w+3 and the same V pieces.
// The DMA writes lane-linear (lane l -> key l >> 4 of the piece, 16-byte position l & 15), so the XOR swizzles of the
// images are applied to the per-lane SOURCE chunk.  No staging registers, no ds_write pass; keys beyond the sequence
// are clamped to its last row (finite data; their scores are masked, their probabilities are 0).
// scalar base (advances by one tile) + per-lane 32-bit byte offset (constant): no per-lane 64-bit arithmetic per piece
__device__ __forceinline__ void dma16(u32 voff, const void* sbase, u32 lds_addr) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(sbase), "s"(lds_addr) : "memory");
}
__device__ __forceinline__ void tiles_landed() {      // every wave's pieces: own queue drained, then the barrier
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
}

// The fp16 rows of one KV head, key j at base + j * stride (elements), with this lane's source offset - ONE register each for K
// and V (round 6; were PPW each).  Piece i of a wave covers keys 4 (PPW wave + i) + (lane >> 4): the rows of piece i are 4 i keys
// further on - a wave-uniform distance that goes into the scalar base -, the V swizzle depends on key & 3 = (lane >> 4) & 3 only,
// and the K swizzle pos ^ (key & 15) differs between the pieces by an XOR with 4 i on the 16-byte position (PPW = 4:
// key & 15 = 4 i + (lane >> 4)), i.e. by `^ 64 i` on the byte offset - ON THE SUMMED OFFSET only where the row part
// (lane >> 4) * stride * 2 leaves the low 8 bits alone, i.e. for stride % 128 == 0 (whole heads per token: every layout of the
// engine).  Any other K stride (a padded row, a view into a wider buffer) takes the per-piece offsets of stage_fp16_tile's general
// path.  V has no per-piece term: any stride.
struct TileRows {
    const _Float16* base;
    int64_t stride;
    u32 off0;
};
__device__ __forceinline__ TileRows k_rows(const _Float16* base, int64_t stride, int lane) {
    const int l4 = lane >> 4, pos = lane & 15;
    return {base, stride, (u32)l4 * (u32)stride * 2u + (u32)((pos ^ l4) * 16)};
}
__device__ __forceinline__ TileRows v_rows(const _Float16* base, int64_t stride, int lane) {
    const int l4 = lane >> 4, pos = lane & 15;
    return {base, stride, (u32)l4 * (u32)stride * 2u + (u32)((pos ^ (l4 << 2)) * 16)};
}
// keys 64 t .. 64 t + 63 of a sequence of len_k keys into tile buffers `buf`; lds_k = lds_address(smem)
__device__ __forceinline__ void stage_fp16_tile(int t, int buf, int len_k, int wave, u32 lds_k, const TileRows& ks, const TileRows& vs) {
    const u32 lds_v = lds_k + 2 * KS_BYTES;
    const _Float16* kb_ = ks.base + ((size_t)t * BN + 4 * PPW * wave) * ks.stride;   // first key of this wave's pieces
    const _Float16* vb_ = vs.base + ((size_t)t * BN + 4 * PPW * wave) * vs.stride;
    // wave-uniform: the last tile of a sequence, or K rows whose stride the one-register form of k_rows cannot serve (scalar test)
    const bool ragged = t * BN + BN > len_k || (ks.stride & 127) != 0;
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
        if (ragged) {                                 // general per-piece offsets, the row clamped to the sequence's last key (from the TILE's base)
            // (from a lane id of its own: derived from the caller's `lane`, the per-piece offsets of this once-per-workgroup path
            //  are loop invariants the compiler keeps in - and spills from - registers across the key loop)
            const int fl = (int)fresh_lane_id(), l4r = fl >> 4, posr = fl & 15;
            const int key = 4 * (PPW * wave + i) + l4r;
            int kc = len_k - 1 - t * BN;
            kc = key < kc ? key : kc;
            const u32 ko = (u32)kc * (u32)ks.stride * 2u + (u32)((posr ^ (key & 15)) * 16);
            const u32 vo = (u32)kc * (u32)vs.stride * 2u + (u32)((posr ^ ((key & 3) << 2)) * 16);
            dma16(ko, ks.base + (size_t)t * BN * ks.stride, lds_k + buf * KS_BYTES + (PPW * wave + i) * 1024);
            dma16(vo, vs.base + (size_t)t * BN * vs.stride, lds_v + buf * VT_BYTES + (PPW * wave + i) * 1024);
        } else {
            // (the XOR is re-done per tile by an opaque statement: hoisted out of the loop - as the compiler does with the plain
            //  expression - the three extra offsets are exactly what it spills to scratch once O is pinned)
            u32 ko = ks.off0;
            if (i > 0) asm volatile("v_xor_b32 %0, %1, %2" : "=v"(ko) : "n"(64 * i), "v"(ks.off0));
            dma16(ko, kb_ + (size_t)(4 * i) * ks.stride, lds_k + buf * KS_BYTES + (PPW * wave + i) * 1024);
            dma16(vs.off0, vb_ + (size_t)(4 * i) * vs.stride, lds_v + buf * VT_BYTES + (PPW * wave + i) * 1024);
        }
    }
}

// ---------------- S^T = K Q^T : two blocks of 32 keys ----------------
// sacc[kb][r] = score of (this lane's row, key 32kb + (r&3) + 8(r>>2) + 4hi of the tile), unscaled.
// operand reads run one group of 4 MFMAs ahead of the matrix pipe (two register sets): issued as written, they
// leave the compiler no choice but counted lgkmcnt waits - with read-then-use in one loop body every MFMA sat behind
// a full LDS round trip
__device__ __forceinline__ void read_k(const uint8_t* s_k, int lane, int g, h8 (&dst)[4]) {   // group g = (kb = g >> 1, s = 4 (g & 1) .. +3)
    const int li = lane & 31, hi = lane >> 5;
    const int key = 32 * (g >> 1) + li;
    const uint8_t* krow = &s_k[key * 256];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int sl = 4 * (g & 1) + j;
        dst[j] = *reinterpret_cast<const h8*>(krow + (((2 * sl + hi) ^ (key & 15)) * 16));
    }
}
template <class BUF>
__device__ __forceinline__ void qk_tile(const uint8_t* smem, BUF bufc, int lane, const h8 (&qf)[8], v16f (&sacc)[NKB]) {
    const int buf = bufc;
    const uint8_t* s_k = smem + buf * KS_BYTES;
    h8 ka[2][4];
    read_k(s_k, lane, 0, ka[0]);
    read_k(s_k, lane, 1, ka[1]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            // the first MFMA of a 32-key block starts from C = 0 (an inline constant operand: no 16-register zero
            // fill per block and tile)
            const v16f zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            const bool first = (g & 1) == 0 && j == 0;
            sacc[g >> 1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ka[g & 1][j], qf[4 * (g & 1) + j], first ? zero16 : sacc[g >> 1], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (g + 2 < 4) read_k(s_k, lane, g + 2, ka[g & 1]);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// A operands of O^T += V^T P^T by the LDS transpose read: a 16-lane group (16 consecutive dims, one lane half) reads
// the [4 keys][16 dims] block of the row-major tile - lane a supplies the 8-byte piece (key a>>2, dims 4(a&3)..+3) -
// and lane c receives column c = (dim c, keys 0..3), i.e. exactly its four k-slots of the PV MFMA.  Group d = the
// four MFMAs of output dims 32d .. 32d+31; the callers request group 0 under the softmax.
template <class BUF>
__device__ __forceinline__ void read_v(const uint8_t* smem, BUF bufc, int lane, int d, h8 (&dst)[4]) {
    const int buf = bufc;
    const int hi = lane >> 5, ta = lane & 15, g1 = (lane >> 4) & 1;
    const int tkey = 4 * hi + (ta >> 2);                       // key within a 16-key block; tkey & 3 == ta >> 2
    const int chunk = (4 * d + 2 * g1 + ((ta & 3) >> 1)) ^ ((ta >> 2) << 2);   // V image swizzle: chunk ^ 4 (key & 3)
    const uint8_t* s_vt = smem + 2 * KS_BYTES + buf * VT_BYTES;
    const uint8_t* vrow = &s_vt[tkey * 256 + chunk * 16 + (ta & 1) * 8];
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const int kofs = (32 * kb + 16 * m) * 256;
            typedef short s4 __attribute__((ext_vector_type(4)));
            typedef __attribute__((address_space(3))) s4* lds_s4;
            const s4 t0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)(vrow + kofs));             // keys +0..3
            const s4 t1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)(vrow + kofs + 8 * 256));   // keys +8..11
            const v2u lo = __builtin_bit_cast(v2u, t0), hi2 = __builtin_bit_cast(v2u, t1);
            dst[2 * kb + m] = __builtin_bit_cast(h8, (v4u){lo.x, lo.y, hi2.x, hi2.y});
        }
}

// Mask, running maximum, probabilities pb[kb][m] (8 per entry, in B-operand order), running sum and the rescale of O.
// Masking only where the caller says the tile needs it (a wave-uniform test: the tile touches a diagonal or the end of the keys):
// key `key` of the tile counts for this lane's row iff key <= limit_of_row(), which is asked for only where a mask is needed.
// Raw scores stay unscaled, the scale is folded into the exponent's fma.
//  * The comparison is made as `32 kb + (r & 3) + 8 (r >> 2) <= limit - 4 hi`: the lane half goes into the limit and the 32 key
//    indices are immediates.  With the lane half in the key, the keys are 32 loop-invariant registers the compiler hoists out of
//    the key loop: the prefill kernels then need 256 VGPRs and spill (<full, 1> 72 bytes of scratch, <causal, 1> 16).
//  * The mask is marked unlikely (one or two tiles per wave touch the diagonal or the end) so that its 64 compare / select
//    instructions sit out of line: as a block the unmasked path has to jump over, they cost the causal prefill 0.6 % at
//    4 x 8 192 tokens (profiles/flash_tile_refactor.txt).
//  * Mask first, then ONE maximum chain over the masked or untouched scores: with a chain in each branch the compiler copies the
//    32 score registers where the branches meet (32 v_mov_b64 per tile in <full, 1>).  max is exact: the same values.
// LAZY running maximum (round 6) - a row's reference maximum moves only when a tile exceeds it by more than 2^8 (probabilities stay
// <= 256 in fp16, sums in fp32: the same softmax), so the rescale, which ran on ~85 % of the tiles of a 1 024-token prompt,
// becomes rare.  LAZY = false is the exact running maximum of the prefill kernel of rounds 2-5.
// The two mask rules, both with the lane half OUT of the key index (`hi` = lane >> 5 goes into the limit / the word):
//   mask_keys_above  a prefix: key <= limit (causal diagonals, the end of the keys, the end of a page's live slots);
//   mask_keys_by_word  a set: bit `key` of a 64-bit word (the ancestor masks of tree-draft verification, append_tree.hip).
__device__ __forceinline__ void mask_keys_above(v16f (&sacc)[NKB], int limit_of_row, int hi) {
    const int limit = limit_of_row - 4 * hi;
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) sacc[kb][r] = 32 * kb + (r & 3) + 8 * (r >> 2) <= limit ? sacc[kb][r] : -INFINITY;
}
__device__ __forceinline__ void mask_keys_by_word(v16f (&sacc)[NKB], uint64_t word, int hi) {
    static_assert(NKB == 2, "one 32-bit half of the word per 32-key block");
    const uint64_t w = word >> (4 * hi);
    const u32 half[2] = {(u32)w, (u32)(w >> 32)};
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) sacc[kb][r] = (half[kb] & (1u << ((r & 3) + 8 * (r >> 2)))) != 0 ? sacc[kb][r] : -INFINITY;
}

// softmax_tile_masked: the mask is the caller's - mask_tile(sacc, hi) is called only where a mask is needed and applies either rule
// (or picks one by a wave-uniform test); softmax_tile below is the prefix rule, key <= limit_of_row().
template <bool LAZY, class MASK>
__device__ __forceinline__ void softmax_tile_masked(v16f (&sacc)[NKB], bool need_mask, MASK mask_tile, int lane, float scale_log2, float& m_run,
                                                    float& l_run, v16f (&oacc)[4], u32 (&pb)[NKB][2][4]) {
    const int hi = lane >> 5;
    if (__builtin_expect(need_mask, 0)) mask_tile(sacc, hi);
    float mx = -INFINITY;
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sacc[kb][r]);
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64)) * scale_log2;      // scale > 0: max commutes with it
    const float m_new = LAZY ? (mx > m_run + 8.0f ? mx : m_run) : fmaxf(m_run, mx);
    const float m_use = m_new == -INFINITY ? 0.f : m_new;     // fully masked so far: keep exp2 arguments finite
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_use);                  // m_run = -inf -> 0
    m_run = m_new;
    // two scores per instruction where the ISA has a packed form (v_pk_fma_f32, v_pk_add_f32; the exponential has none):
    // round 5, the key loop is as VALU-bound as it is MFMA-bound (HISTORY 5.5)
    typedef float v2f __attribute__((ext_vector_type(2)));
    const v2f sc2 = {scale_log2, scale_log2}, nm2 = {-m_use, -m_use};
    v2f psum2 = {0.f, 0.f};
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const v2f sv = {sacc[kb][8 * m + 2 * j], sacc[kb][8 * m + 2 * j + 1]};
                v2f pp = __builtin_elementwise_fma(sv, sc2, nm2);
                pp[0] = __builtin_amdgcn_exp2f(pp[0]);          // -inf stays -inf -> 0
                pp[1] = __builtin_amdgcn_exp2f(pp[1]);
                psum2 += pp;
                pb[kb][m][j] = pack_h2(pp[0], pp[1]);
            }
    const float psum = psum2[0] + psum2[1];
    l_run = l_run * alpha + psum;
    // (LAZY: marked unlikely - with the lazy maximum it is the first tile and jumps of more than 2^8.  The not-taken path must not
    //  carry register copies of the 64 accumulators: see the loop structure of the callers)
    if (LAZY ? __builtin_expect(__any(alpha != 1.0f), 0) : __any(alpha != 1.0f)) {   // the running max moved for some row of this wave
#pragma unroll
        for (int d = 0; d < 4; ++d)
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[d][r] *= alpha;
    }
}

template <bool LAZY, class LIMIT>
__device__ __forceinline__ void softmax_tile(v16f (&sacc)[NKB], bool need_mask, LIMIT limit_of_row, int lane, float scale_log2, float& m_run,
                                             float& l_run, v16f (&oacc)[4], u32 (&pb)[NKB][2][4]) {
    softmax_tile_masked<LAZY>(sacc, need_mask, [&](v16f (&s)[NKB], int hi) { mask_keys_above(s, limit_of_row(), hi); }, lane, scale_log2, m_run,
                              l_run, oacc, pb);
}

// ---------------- O^T += V^T P^T ----------------
// va[0] holds group 0 (read_v(..., 0, va[0]), requested by the caller in front of the softmax); the further groups are read here,
// one group of 4 MFMAs ahead
template <class BUF>
__device__ __forceinline__ void pv_tile(const uint8_t* smem, BUF bufc, int lane, h8 (&va)[2][4], const u32 (&pb)[NKB][2][4], v16f (&oacc)[4]) {
    read_v(smem, bufc, lane, 1, va[1]);
    __builtin_amdgcn_sched_barrier(0);
    static_for<4>([&](auto dc) {
        constexpr int d = decltype(dc)::value;
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                const h8 pbv = __builtin_bit_cast(h8, (v4u){pb[kb][m][0], pb[kb][m][1], pb[kb][m][2], pb[kb][m][3]});
                oacc[d] = __builtin_amdgcn_mfma_f32_32x32x16_f16(va[d & 1][2 * kb + m], pbv, oacc[d], 0, 0, 0);
            }
        __builtin_amdgcn_sched_barrier(0);
        if (d + 2 < 4) read_v(smem, bufc, lane, d + 2, va[d & 1]);
        __builtin_amdgcn_sched_barrier(0);
    });
}

// Epilogue (round 6): O, normalised by `inv` and rounded to fp16, goes through LDS and leaves as WHOLE ROWS.  In the accumulator
// layout a lane owns one query row, so the direct form is 16 stores of 8 bytes per lane at a row stride (8 KiB for 32 heads): every
// store instruction touches 64 different cache lines, and the store tail of a workgroup lasts ~2 key tiles (MI355X_MICROARCH.md:
// "attention epilogue store tail ... store-ISSUE-bound").  Here a wave writes its 32 x 128 fp16 block into its own 8.5 KiB of the
// (dead) K / V buffers - row stride 272 B: the rows of a half-wave fall on banks 4 li, two-way conflicts at most - and reads it back
// 16 bytes per lane, 16 lanes per row: 8 stores per lane, each instruction 4 complete 256-byte rows.  No barrier: every wave has
// passed the last tile's barrier (all reads of the buffers are over) and touches only its own block; the LDS serves a wave's accesses
// in order.  put(r, cc, x) stores the 16-byte chunk cc (dims 8 cc .. + 7) of row r (0 .. 31) of this wave, or drops it where the
// row is not one to store: the caller owns the row mapping and its bounds.
// (the lane ids are re-derived: kept alive across the key loop they cost registers the causal prefill instantiation does not have)
template <class PUT>
__device__ __forceinline__ void store_rows_through_lds(uint8_t* smem, int wave, const v16f (&oacc)[4], float inv, PUT put) {
    uint8_t* const so = smem + wave * (32 * OST);
    const int li_e = (int)(fresh_lane_id() & 31u), hi_e = (int)(fresh_lane_id() >> 5);
    static_for<4>([&](auto dc) {
        constexpr int d = decltype(dc)::value;
        static_for<4>([&](auto rc) {
            constexpr int rq = decltype(rc)::value;
            h4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = (_Float16)(oacc[d][4 * rq + j] * inv);
            *reinterpret_cast<h4*>(so + li_e * OST + (32 * d + 8 * rq + 4 * hi_e) * 2) = o;
        });
    });
    const int lid = (int)fresh_lane_id(), rr = lid >> 4, cc = lid & 15;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int r = 4 * j + rr;
        put(r, cc, *reinterpret_cast<const v4u*>(so + r * OST + cc * 16));
    }
}

}  // namespace qs_flash
