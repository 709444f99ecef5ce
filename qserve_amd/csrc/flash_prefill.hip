// flash_prefill.hip -- prefill attention (causal / full, variable-length, GQA, fp16, head_dim 128) for MI355X (gfx950).
//
// Provider for the call the reference makes into the un-vendored flash-attn package
//   flash_attn.flash_attn_interface.flash_attn_varlen_func(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q,
//   max_seqlen_k, causal=True)            (qserve/modeling/models/llama_w4a8_unpad.py:30,232-242)
// flash-attn v2 semantics: softmax(scale * Q K^T) V per sequence and head, fp32 softmax, causal mask aligned to the
// bottom-right corner when the query and key lengths differ.  The algorithm is the published FlashAttention-2 forward
// (online softmax over key tiles, no S x S matrix).  The mapping onto CDNA4 - 64-key tiles of K and V in LDS, swapped products on
// v_mfma_f32_32x32x16_f16, register-only softmax, O out through LDS as whole rows - is the tile core of flash_tile.h, shared with
// append_attention.hip; what this file adds is WHO the rows are and the tile schedule:
//   * workgroup = 4 wave64 = 128 query rows of one (sequence, head); wave w owns 32 rows and keeps their Q fragments
//     (8 x 16 dims) in registers for the whole key loop;
//   * the tiles are the fp16 k / v rows of the sequence, staged once per workgroup (the G query heads of a GQA group are separate
//     workgroups that re-read the tiles from L2), up to the causal diagonal of the workgroup's last row.
#include "flash_tile.h"

namespace {

using namespace qs_flash;

#ifdef QS_FLASH_TRACE
// timing builds only (scripts/trace_flash.py): cycles per phase of the key loop, summed per wave
__device__ unsigned long long* g_flash_trace = nullptr;
#define QS_FT(i) do { const unsigned long long n_ = __builtin_amdgcn_s_memtime(); ft[i] += (unsigned)(n_ - ft_t); ft_t = n_; } while (0)
#else
#define QS_FT(i) do { } while (0)
#endif

// VAR = 1 (round 6, the default) against VAR = 0 (the kernel of rounds 2-5, kept for the A/B: qs_debug_flash_variant(1)):
//  (1) the Q fragments are complete FOR THE COMPILER before the key loop: it had kept them "load pending" and put counted vmcnt
//      waits in front of the first Q.K^T MFMAs of every tile - waits that also drain the LDS-DMA of tile t + 1, issued a few
//      instructions earlier by asm it does not see.  Every wave sat through the L2 round trip of its own prefetch, every tile;
//  (2) no register copies of the O accumulators in the key loop: 32 v_mov_b64 per tile and wave came from two control-flow merges
//      the 64 accumulators were carried through - the rescale branch (now marked unlikely: its copies live on the cold path) and the
//      skip of fully masked causal tiles (now a loop of its own behind the computing loop).  Pinning O to fixed registers through
//      asm (physical-register constraints) and asm-owned accumulator registers were tried first: the former spills 30 registers in
//      the loop, the latter makes the compiler split the wave's 256 registers 128 / 128 and move the score tiles into AGPRs;
//  (3) LAZY running maximum - a row's reference maximum moves only when a tile exceeds it by more than 2^8 (probabilities stay
//      <= 256 in fp16, sums in fp32: the same softmax), so the rescale, which ran on ~85 % of the tiles of a 1 024-token prompt,
//      becomes rare;
//  (4) the tile loop unrolled by two with the LDS buffer index a compile-time constant (every ds_read address a loop-invariant
//      register + an immediate offset; the loop carried ~47 v_add_u32 of address arithmetic per tile and wave);
//  (5) O leaves through LDS as whole rows (see the epilogue).
// In-run A/B (profiles/round6_flash_ab7.txt): 64 x 1 024 tokens 0.233 -> 0.277 of the dense fp16 MFMA peak, 4 x 8 192: 0.345 -> 0.397.
template <bool CAUSAL, int VAR>
__global__ __launch_bounds__(64 * NWV, 2) void flash_fwd_kernel(const _Float16* __restrict__ q, const _Float16* __restrict__ k,
                                                          const _Float16* __restrict__ v, _Float16* __restrict__ out,
                                                          const int* __restrict__ cu_q, const int* __restrict__ cu_k,
                                                          int num_heads, int num_kv_heads, int64_t q_stride0,
                                                          int64_t k_stride0, int64_t v_stride0, int64_t o_stride0,
                                                          float scale_log2) {
    constexpr bool R6 = VAR != 0;      // VAR: 0 = the kernel of rounds 2-5 (A/B: qs_debug_flash_variant(1)), 1 = round 6 (default)
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // grid = (heads, query tiles, sequences).  All workgroups of ONE sequence are dispatched next to each other (its K / V -
    // 0.5 MB per KV head at 1024 tokens - are fetched from HBM once and re-served by L2 / the Infinity Cache to its
    // query tiles and heads), inside a sequence the query tiles run last-to-first for causal launches (the workgroups that
    // see the most keys start first: longest-first keeps the tail short), and the head index is permuted so that
    // workgroups 8 apart - which share an XCD and its L2 - are the G heads of one KV group.
    // (measured at 64 x 1024 / 4 x 8192 tokens: query tile fastest 417 / 740 TFLOP/s, query tile slowest 449 / 822, this
    //  order 508 / 858)
    const int b = blockIdx.z, qt = CAUSAL ? (int)(gridDim.y - 1 - blockIdx.y) : (int)blockIdx.y;
    const int h = (int)(blockIdx.x % num_kv_heads) * (num_heads / num_kv_heads) + (int)(blockIdx.x / num_kv_heads);
    const int q_start = cu_q[b], len_q = cu_q[b + 1] - q_start;
    const int k_start = cu_k[b], len_k = cu_k[b + 1] - k_start;
    if (qt * BM >= len_q) return;
    const int hkv = h / (num_heads / num_kv_heads);
    const int shift = len_k - len_q;                   // causal diagonal: key <= row + shift
    const int li = lane & 31, hi = lane >> 5;
    const int row = qt * BM + wave * 32 + li;          // this lane's query row (both lane halves share it)
    const int row_ld = row < len_q ? row : len_q - 1;

    // ---- Q fragments: B operand of S^T = K Q^T, lane (row, hi) holds dims 16s + 8hi .. +8 ----------------------------
    h8 qf[8];
    {
        const _Float16* qp = q + (size_t)(q_start + row_ld) * q_stride0 + (size_t)h * DH + 8 * hi;
#pragma unroll
        for (int s = 0; s < 8; ++s) qf[s] = *reinterpret_cast<const h8*>(qp + 16 * s);
    }

    // ---- key range ----------------------------------------------------------------------------------------------------
    int kv_end = len_k;
    if (CAUSAL) {
        const int last = qt * BM + BM - 1 + shift;     // largest key any row of this workgroup may see
        kv_end = last + 1 < len_k ? last + 1 : len_k;
    }
    const int ntiles = kv_end > 0 ? (kv_end + BN - 1) / BN : 0;

    // ---- tile staging by LDS-DMA (stage_fp16_tile): the k / v rows of this sequence and KV head
    const TileRows ksrc = k_rows(k + (size_t)k_start * k_stride0 + (size_t)hkv * DH, k_stride0, lane);
    const TileRows vsrc = v_rows(v + (size_t)k_start * v_stride0 + (size_t)hkv * DH, v_stride0, lane);
    const u32 lds_k = lds_address(smem);
    auto load_tile = [&](int t, int buf) { stage_fp16_tile(t, buf, len_k, wave, lds_k, ksrc, vsrc); };

    v16f oacc[4];
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[d][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;

    if (ntiles > 0) load_tile(0, 0);
    // The Q fragments must be COMPLETE FOR THE COMPILER before the key loop (round 6).  They come from ordinary global loads; the
    // only wait in front of the loop was the asm vmcnt(0) of tiles_landed(), which the compiler's wait-count pass does not see - so
    // it kept the fragments "load pending" into the loop and put counted waits in front of the first Q.K^T MFMAs of EVERY tile
    // (s_waitcnt vmcnt(7) ... vmcnt(0), one per fragment).  The hardware counter it waits on also counts the LDS-DMA of tile
    // t + 1, issued a few instructions earlier by asm the compiler does not see either: every wave sat through the L2 round trip
    // of its own prefetch inside Q.K^T of every tile (the "1 430 cycles for DMA issue + Q.K^T" of the round-2 trace, 512 of them
    // MFMA).  An empty asm that rewrites the fragments makes the compiler wait HERE, once (tests/test_kernel_contracts.py pins:
    // no vmcnt wait between the loop's barriers other than the explicit one of tiles_landed()).
    if constexpr (R6) {
#pragma unroll
        for (int s = 0; s < 8; ++s) asm volatile("" : "+v"(qf[s]));
    }
    tiles_landed();

#ifdef QS_FLASH_TRACE
    unsigned ft[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long ft_t = __builtin_amdgcn_s_memtime();
#endif
    // one tile; BUFC = std::integral_constant<int, 0 / 1> (R6: the buffer index is a compile-time constant) or a run-time int
    auto tile_body = [&](auto bufc, int t) {
        const int buf = bufc;
        QS_FT(0);
        // (round 6, measured and dropped: the pieces of tile t + 1 requested LATER - K behind Q.K^T, V behind the exponentials, where an
        //  LDS-DMA instruction should cost the wave fewer issue cycles than next to 16 ds_read_b128: equal at 64 x 1 024 tokens, -0.8 %
        //  at 4 x 8 192, profiles/round6_flash_ab6.txt)
        if (t + 1 < ntiles) load_tile(t + 1, buf ^ 1);   // lands in the other buffers during this tile
        // causal: the workgroup's key range ends at its LAST row's diagonal; a wave whose 32 rows all lie before this tile
        // has nothing to add (every score masked) - it only takes part in the staging and the barrier
        // (R6: such tiles never reach this body - see the loops below)
        if (!R6 && CAUSAL && t * BN > qt * BM + wave * 32 + 31 + shift) {
            tiles_landed();
            return;
        }

        v16f sacc[NKB];
        qk_tile(smem, bufc, lane, qf, sacc);
        QS_FT(1);                                                  // DMA issue + Q.K^T
        h8 va[2][4];
        read_v(smem, bufc, lane, 0, va[0]);                        // group 0 of the P.V operands, requested under the softmax
        __builtin_amdgcn_sched_barrier(0);
        // masking only where the tile touches the diagonal or the end of the keys (wave-uniform test); `limit` = the last key of
        // the tile this lane's row may see
        const int tile_last = t * BN + BN - 1;
        const bool need_mask = tile_last >= len_k || (CAUSAL && tile_last > qt * BM + wave * 32 + shift);
        auto limit = [&] { return (CAUSAL && row + shift < len_k - 1 ? row + shift : len_k - 1) - t * BN; };
        u32 pb[NKB][2][4];
        softmax_tile<R6>(sacc, need_mask, limit, lane, scale_log2, m_run, l_run, oacc, pb);   // R6: lazy reference maximum (see the kernel's header)
        QS_FT(2);                                                  // mask + softmax + O rescale
        pv_tile(smem, bufc, lane, va, pb, oacc);
        QS_FT(3);                                                  // P.V
        tiles_landed();
        QS_FT(4);                                                  // wait for the next tile + barrier
    };
    if constexpr (R6) {
        // tiles this WAVE computes: a causal tile whose first key lies beyond the wave's last row has nothing to add - for those
        // the wave only takes part in the staging and the barrier (second loop).  Kept out of the first loop on purpose: a skip
        // path that rejoins the computing path inside the loop is a control-flow merge the 64 O accumulators are carried
        // through, and the compiler resolves such merges with register copies.
        int nt_w = ntiles;
        if (CAUSAL) {
            const int last_key = qt * BM + wave * 32 + 31 + shift;
            nt_w = last_key < 0 ? 0 : min(ntiles, last_key / BN + 1);
        }
        int t = 0;
        for (; t + 1 < nt_w; t += 2) {
            tile_body(std::integral_constant<int, 0>(), t);
            tile_body(std::integral_constant<int, 1>(), t + 1);
        }
        if (t < nt_w) {
            tile_body(std::integral_constant<int, 0>(), t);
            ++t;
        }
        for (; t < ntiles; ++t) {
            if (t + 1 < ntiles) load_tile(t + 1, (t + 1) & 1);
            tiles_landed();
        }
    } else {
        for (int t = 0; t < ntiles; ++t) tile_body(t & 1, t);
    }
#ifdef QS_FLASH_TRACE
    if (g_flash_trace && lane == 0) {
        unsigned long long* o = g_flash_trace + ((((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * NWV + wave) * 8;
        for (int i = 0; i < 5; ++i) o[i] = ft[i];
        o[5] = ntiles;
    }
#endif

    // ---- epilogue: normalise, fp16 ----------------------------------------------------------------------------------------
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    const float inv = l_tot > 0.f ? 1.0f / l_tot : 0.f;
    // (the row index is re-derived from a lane id the compiler cannot merge with the one above: kept alive across the key loop
    //  it costs a register the causal instantiation does not have)
    const int row_e = qt * BM + wave * 32 + (int)(fresh_lane_id() & 31u);
    // whole-row stores need 16-byte alignment of every row (wave-uniform)
    const bool rows16 = R6 && (o_stride0 % 8 == 0) && ((reinterpret_cast<uintptr_t>(out) & 15) == 0);
    if (rows16) {
        // out through LDS as whole 256-byte rows (store_rows_through_lds): row r of this wave is query row row0 + r of head h
        const int row0 = qt * BM + wave * 32;
        _Float16* const ob = out + (size_t)(q_start + row0) * o_stride0 + (size_t)h * DH;
        store_rows_through_lds(smem, wave, oacc, inv, [&](int r, int cc, const v4u& x) {
            if (row0 + r < len_q) *reinterpret_cast<v4u*>(ob + (size_t)r * o_stride0 + cc * 8) = x;
        });
    } else if (row_e < len_q) {
        // 8-byte stores (4 consecutive dims per accumulator quad)
        _Float16* op = out + (size_t)(q_start + row_e) * o_stride0 + (size_t)h * DH;
        static_for<4>([&](auto dc) {
            constexpr int d = decltype(dc)::value;
            static_for<4>([&](auto rc) {
                constexpr int rq = decltype(rc)::value;
                h4 o;
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = (_Float16)(oacc[d][4 * rq + j] * inv);
                *reinterpret_cast<h4*>(op + 32 * d + 8 * rq + 4 * hi) = o;
            });
        });
    }
}

}  // namespace

#ifdef QS_FLASH_TRACE
extern "C" int qs_debug_flash_trace(void* buf) {
    unsigned long long* p = reinterpret_cast<unsigned long long*>(buf);
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_flash_trace), &p, sizeof(p));
}
#endif

static qs_flag g_flash_variant = 0;
// A/B hook (include/qserve_amd.h): 0 = lazy running maximum + tile loop unrolled over the two LDS buffers (round 6, default),
// 1 = the loop of rounds 2-5.  The same softmax; the reference maximum differs, so low-order bits may.
extern "C" int qs_debug_flash_variant(int variant) {
    QS_REQUIRE(variant == 0 || variant == 1, "qs_debug_flash_variant: %d not in {0, 1}", variant);
    g_flash_variant = variant;
    return QS_OK;
}

extern "C" int qs_flash_attn_varlen_fwd(const void* q, const void* k, const void* v, void* out,
                                        const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k, int batch,
                                        int num_heads, int num_kv_heads, int head_dim, int64_t q_stride0,
                                        int64_t k_stride0, int64_t v_stride0, int64_t o_stride0, int max_seqlen_q,
                                        int max_seqlen_k, float softmax_scale, int causal, qs_stream_t stream) {
    QS_REQUIRE(q && k && v && out && cu_seqlens_q && cu_seqlens_k, "flash_attn_varlen: null pointer");
    QS_REQUIRE(batch >= 0 && num_heads > 0 && num_kv_heads > 0 && num_heads % num_kv_heads == 0,
               "flash_attn_varlen: bad head counts H=%d Hkv=%d", num_heads, num_kv_heads);
    if (head_dim != DH) {
        qs_set_error("flash_attn_varlen: head_dim=%d, only 128 is supported (the reference's models)", head_dim);
        return QS_ENOSUP;
    }
    // The layouts the kernels serve (include/qserve_amd.h) - everything else is refused HERE, in front of every device call:
    // q / k / v rows are read 16 bytes at a time (k / v by LDS-DMA with 32-bit lane offsets of up to 64 rows), out is written 16 bytes
    // at a time where its base and stride allow it and 8 bytes at a time otherwise.
    QS_REQUIRE(q_stride0 % 8 == 0 && k_stride0 % 8 == 0 && v_stride0 % 8 == 0 && o_stride0 % 4 == 0,
               "flash_attn_varlen: token strides must keep 16-byte alignment");
    QS_REQUIRE(q_stride0 >= (int64_t)num_heads * DH && o_stride0 >= (int64_t)num_heads * DH && k_stride0 >= (int64_t)num_kv_heads * DH &&
                   v_stride0 >= (int64_t)num_kv_heads * DH,
               "flash_attn_varlen: a token stride is shorter than the token's heads");
    QS_REQUIRE(q_stride0 < (1 << 24) && k_stride0 < (1 << 24) && v_stride0 < (1 << 24) && o_stride0 < (1 << 24),
               "flash_attn_varlen: token strides must be below 2^24 elements");
    QS_REQUIRE(((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(v)) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(out) & 7) == 0,
               "flash_attn_varlen: q, k, v must be 16-byte aligned and out 8-byte aligned");
    QS_REQUIRE(max_seqlen_q >= 0 && max_seqlen_k >= 0, "flash_attn_varlen: negative max_seqlen");
    QS_REQUIRE(softmax_scale > 0.f, "flash_attn_varlen: softmax_scale must be positive");
    if (batch == 0 || max_seqlen_q == 0) return QS_OK;
    const float scale_log2 = softmax_scale * 1.4426950408889634f;
    dim3 grid(num_heads, (max_seqlen_q + BM - 1) / BM, batch);
    constexpr int SMEM = 2 * KS_BYTES + 2 * VT_BYTES;   // dynamic LDS: K [2][16 KiB], then V [2][16 KiB] (flash_tile.h)
    static bool lds_reserved[QS_MAX_DEVICES] = {};
    if (const hipError_t e = qs_reserve_lds({reinterpret_cast<const void*>(flash_fwd_kernel<true, 0>), reinterpret_cast<const void*>(flash_fwd_kernel<true, 1>),
                                             reinterpret_cast<const void*>(flash_fwd_kernel<false, 0>), reinterpret_cast<const void*>(flash_fwd_kernel<false, 1>)},
                                            SMEM, lds_reserved); e != hipSuccess) {
        qs_set_error("flash_attn_varlen: cannot reserve %d bytes of LDS", SMEM);
        return (int)e;
    }
#define QS_FL(C, P)                                                                                                    \
    hipLaunchKernelGGL((flash_fwd_kernel<C, P>), grid, dim3(64 * NWV), SMEM, (hipStream_t)stream, (const _Float16*)q,   \
                       (const _Float16*)k, (const _Float16*)v, (_Float16*)out, cu_seqlens_q, cu_seqlens_k, num_heads,  \
                       num_kv_heads, q_stride0, k_stride0, v_stride0, o_stride0, scale_log2)
    if (causal) {
        if (g_flash_variant == 0) QS_FL(true, 1);
        else QS_FL(true, 0);
    } else {
        if (g_flash_variant == 0) QS_FL(false, 1);
        else QS_FL(false, 0);
    }
#undef QS_FL
    return qs_launch_status("flash_attn_varlen");
}
