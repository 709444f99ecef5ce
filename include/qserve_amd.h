/*
 * qserve_amd.h -- C ABI of libqserve_amd.so: MI355X (gfx950) implementation of QServe's W4A8KV4 hot path.
 *
 * This is the drop-in boundary.  Every entry point below is what the reference's pybind11 torch-extension
 * functions (package `qserve_backend`, kernels/setup.py:157-245) reduce to once the torch::Tensor arguments
 * are lowered to device pointers + sizes.  The Python package `qserve_backend/` in this repository is the
 * host-side mirror that performs exactly that lowering (same module names, same callables, same argument
 * order and error behaviour); INTEGRATION.md shows the binding a maintainer of the reference would add.
 *
 * Conventions
 *   - all pointers are DEVICE pointers unless stated otherwise; `half` data is passed as `const void*`/`void*`
 *     to IEEE binary16 storage (the ABI carries no torch / HIP types);
 *   - `stream` is a hipStream_t passed as void* (NULL = legacy default stream, which is what the reference
 *     GEMMs use: gemm_cuda.cu:53);
 *   - return value: 0 on success, a negative QS_E* code on rejected arguments (nothing was launched),
 *     a positive hipError_t if the launch failed.  qs_last_error() returns a thread-local message;
 *   - callers own every tensor buffer (ownership rules of the reference, SURVEY.md 8(b) "Conventions"); the library
 *     keeps a few device scratch areas of its own (RoPE cos/sin tables, split-KV partials, split-K slabs - 2 x 48 MiB, one of
 *     them sentinel-filled between launches -, the split argmax's keys / tickets, the generation words and exchange rows of
 *     the fused attention quantiser - 64 MiB, batches up to 4096 sequences, larger ones run the un-fused pair).  Each
 *     is a fixed-size allocation made lazily on a first EAGER call (never while the stream is being captured into a
 *     graph: such a call runs the variant that needs no scratch) and is NEVER freed, moved or grown afterwards, so a
 *     hipGraph that captured its address stays valid for the life of the process.  Requests beyond the fixed capacity
 *     fall back to the un-split variants.  The scratch areas exist once per device (the CURRENT device of the calling thread),
 *     shared by every stream: launches that use them (split-KV attention, K-sliced GEMMs, the split argmax, the fused attention
 *     quantiser's hand-over) must not run concurrently on different streams of one device (the reference's engine is
 *     single-stream) - UNLESS the extra streams were given scratch of their own with qs_stream_scratch_bind() (below: up to 7
 *     streams per device; launches issued on, or captured on, a bound stream use that stream's areas).
 *     A launch that is ABORTED mid-way (device reset) may leave the K-slice slabs without their sentinel or an exchange row
 *     half-tagged: call qs_device_reset() before the library is used again.  The in-launch waits on these areas are BOUNDED
 *     (round 5): a violated assumption yields a status bit (qs_device_status) and an invalid result, never a hung GPU.
 */
#ifndef QSERVE_AMD_H
#define QSERVE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QS_OK 0
#define QS_EINVAL (-1)   /* bad shape / alignment / null pointer */
#define QS_ENOSUP (-2)   /* combination the reference never instantiates (e.g. head_dim != 128) */

typedef void* qs_stream_t;

/* Library identification: version = 100*major + minor; arch string is "gfx950". */
int qs_version(void);
const char* qs_arch(void);
const char* qs_last_error(void);

/* ------------------------------------------------------------------------------------------------------------
 * W4A8 per-channel GEMM.
 * Replaces qserve_backend.qgemm_w4a8_per_chn.gemm_forward_cuda
 *   (kernels/csrc/qgemm/w4a8_per_chn/gemm_cuda.h:11, gemm_cuda.cu:596-652, pybind.cpp:13-16).
 *   in_feats  int8  [M,K] row-major          kernel   int8 [N,K/2]  reference packed layout (w4a8_linear.py:290-322)
 *   wscales   half  [N]                       ascales  half [M]
 *   w_szs     half  [N]  (= zero*scale)       a_ssums  half [M]  (= sum_k x)
 *   out_feats half  [M,N] written in place:   (float(acc)*wscale[n])*ascale[m] - w_sz[n]*a_ssum[m]
 * Requirements: N % 64 == 0, K % 128 == 0 (the reference requires N % CTA_N, K % CTA_K; all model shapes comply).
 * ---------------------------------------------------------------------------------------------------------- */
int qs_w4a8_per_chn_gemm(const int8_t* in_feats, const int8_t* kernel, const void* wscales, const void* ascales,
                         const void* w_szs, const void* a_ssums, void* out_feats, int M, int N, int K,
                         qs_stream_t stream);

/* W4A8 per-group (g128) GEMM.
 * Replaces qserve_backend.qgemm_w4a8_per_group.gemm_forward_cuda
 *   (kernels/csrc/qgemm/w4a8_per_group/gemm_cuda.h:11, gemm_cuda.cu:630-702).
 *   zeros, scales_i8  int8 [K/128, N] in the reference's per-32 channel permutation (w4a8_linear.py:231-277)
 *   out = float(acc) * (wscale[n]*ascale[m]),  acc over the level-2 dequantised int8 weights. */
int qs_w4a8_per_group_gemm(const int8_t* in_feats, const int8_t* kernel, const int8_t* zeros,
                           const int8_t* scales_i8, const void* wscales, const void* ascales, void* out_feats,
                           int M, int N, int K, qs_stream_t stream);

/* gate_up GEMM + silu_and_mul in one launch (engine-side fusion, like the pairs further down; no reference op of its
 * own: LlamaMLP.forward, llama_w4a8_unpad.py:69-93, issues gate_up_proj, then SiluAndMulQuant = silu_and_mul ; invoke_quant).
 *   kernel   the stacked gate_up weight [N, K/2], rows 0 .. N/2-1 = gate, N/2 .. N-1 = up (load_weights' row
 *            concatenation), consumed unchanged;   out_act half [M, N/2];
 *   out_act[m, c] = half(float(silu_h(Y[m, c])) * float(Y[m, N/2 + c]))  with Y = the fp16 result of the plain GEMM entry
 *            above on the same arguments - i.e. bit-identical to  qs_w4a8_*_gemm(..., tmp) ; qs_silu_and_mul(out_act, tmp).
 *   tmp      half [M, N] scratch or NULL: shapes whose kernel family has no activation epilogue (K-sliced geometries,
 *            the round-1 kernels) run as those two launches through it; NULL makes them an error.
 * Requirements: those of the plain entries and N % 128 == 0. */
int qs_w4a8_per_chn_gemm_silu_mul(const int8_t* in_feats, const int8_t* kernel, const void* wscales,
                                  const void* ascales, const void* w_szs, const void* a_ssums, void* out_act, void* tmp,
                                  int M, int N, int K, qs_stream_t stream);
int qs_w4a8_per_group_gemm_silu_mul(const int8_t* in_feats, const int8_t* kernel, const int8_t* zeros,
                                    const int8_t* scales_i8, const void* wscales, const void* ascales, void* out_act,
                                    void* tmp, int M, int N, int K, qs_stream_t stream);

/* Debug/parity entry points: same kernels, but the raw INT32 accumulators are written to acc_out [M,N]
 * instead of the fp16 epilogue (the reference keeps them in registers: gemm_cuda.cu:327). */
int qs_w4a8_per_chn_gemm_acc(const int8_t* in_feats, const int8_t* kernel, int32_t* acc_out, int M, int N, int K,
                             qs_stream_t stream);
int qs_w4a8_per_group_gemm_acc(const int8_t* in_feats, const int8_t* kernel, const int8_t* zeros,
                               const int8_t* scales_i8, int32_t* acc_out, int M, int N, int K, qs_stream_t stream);

/* K-slice PLANES (engine-side pair fusion, round 4): the row-parallel GEMMs of a layer (o_proj, down_proj) are followed by a row
 * kernel that reads their whole output (residual add + norm + quant, llama_w4a8_unpad.py:345-361).  In this form the GEMM leaves
 * the int32 partial sums of its K slices as planes [k_slices][M][N] - no cross-workgroup reduction, no epilogue - and
 * qs_add_residual_rms_norm_general_planes (below) sums them and applies the GEMM's epilogue arithmetic itself, bit for bit.
 *   qs_w4a8_gemm_planes_plan: plan4 = {k_slices, m_tiles, units, token_blocks} the planes launch of this shape will use;
 *                             k_slices == 0: no such launch for this shape (run the ordinary pair).  Deterministic in the shape.
 *   planes: int32 [k_slices][M][N], 16-byte aligned; every element of every plane is written. */
int qs_w4a8_gemm_planes_plan(int per_group, int M, int N, int K, int* plan4);
int qs_w4a8_per_chn_gemm_planes(const int8_t* in_feats, const int8_t* kernel, int32_t* planes, int M, int N, int K,
                                qs_stream_t stream);
int qs_w4a8_per_group_gemm_planes(const int8_t* in_feats, const int8_t* kernel, const int8_t* zeros, const int8_t* scales_i8,
                                  int32_t* planes, int M, int N, int K, qs_stream_t stream);

/* W8A8 GEMM (importable-module requirement only).
 * Replaces qserve_backend.qgemm_w8a8.w8a8_gemm_forward_cuda (kernels/csrc/qgemm/w8a8/w8a8_gemm_cuda.h:11).
 *   kernel int8 [N,K] row-major.  out = float(acc) * (wscale[n]*ascale[m]).  N % 16 == 0, K % 64 == 0. */
int qs_w8a8_gemm(const int8_t* in_feats, const int8_t* kernel, const void* wscales, const void* ascales,
                 void* out_feats, int M, int N, int K, qs_stream_t stream);

/* Kernel-variant selection for benchmarking / A-B tests (process-wide; default -1 = the measured heuristic).  Like every
 * qs_set_* / qs_debug_* switch of this header it is a relaxed atomic inside the library: setting it while another host thread
 * launches is not a data race - that launch sees the old or the new value -, but it is one value for the whole process, not a
 * per-stream or per-thread configuration.  EVERY
 * variant of the shipped library computes the same results; the timing experiments that switch kernel parts off (wrong
 * results by design) exist only in libraries built with -DQS_TIMING (python -m qserve_amd.build --timing ->
 * libqserve_amd_timing.so, loaded by the measurement scripts through QS_AMD_LIBRARY) and are ignored otherwise:
 *   9xx / 1000 + 100*mtile + 10*S + NW ... split-K decode kernel geometries;  2000 / 2001 ... LDS-pair kernel off / forced;
 *   3000 ... tiled (prefill) kernel off, 3001 / 3002 ... forced with the 256- / 128-token tile;
 *   4000 ... ring (decode) kernel off, 4001 ... ring kernel without K slices, 4002 ... cost model without the per-group term,
 *   4004 ... without the 128-token ring geometry <8,2> (round 5),
 *   4600 + 100*(k_slices-1) + 10*m_tiles + units ... forced geometry of the K-slice planes launches,
 *   3003 ... the four-wave compute-bound tile forced (3001: the eight-wave one), 3400 + bits ... [QS_TIMING builds] its ablations,
 *   4100 + 100*(k_slices-1) + 10*m_tiles + units ... forced ring geometry;
 *   5000 + bits ... A/B switches of the ring kernel (1: weight DMA without the non-temporal hint; 256 * d: ring depth d;
 *                   4096: K slices of a channel block on ONE XCD, the mapping of rounds 3-5 - default since round 6: slices across the
 *                   XCDs so that an L2 holds only its K slice of the activations;
 *                   [QS_TIMING builds: 32 / 64 no MFMA / no operand reads]); sticky until reset with 5000;
 *   3200 + 10*p + o ... tiled kernel A/B, sticky until reset with 3200: tile order o (0 super-tiles with the XCD-aware 4 x 8
 *                   placement inside a super-tile, 3 super-tiles without it, 1 / 2 token- / channel-fastest bands); p = 1 one
 *                   workgroup per tile instead of one per CU walking the tiles,
 *                   p = 2 three workgroups walk all tiles (tests of the tile-to-tile hand-over);
 *   3301 / 3300 ... qs_w4a8_*_gemm_silu_mul always as two launches / default (sticky);
 *   3100 + bits ... [QS_TIMING builds only] kernel parts of the tiled kernel switched off. */
void qs_set_gemm_variant(int variant);

/* The codes above by name (round 6; the dispatcher in qserve_amd/csrc/gemm_w4a8.hip uses these, nothing else defines them).
 * The selection state is PROCESS-GLOBAL and NOT THREAD-SAFE: a test / measurement hook, set between launches by one host
 * thread; a serving process never calls it.  Codes that pick a kernel are remembered until the next call; the sticky families
 * (ring flags, tile order, activation split) keep their own word and are reset by their family's base code. */
enum qs_gemm_variant_code {
    QS_GEMM_DEFAULT = -1,              /* the measured heuristic */
    QS_GEMM_SPLITK_BASE = 1000,        /* + 100 * m_tiles + 10 * cross_block_slices + waves: round-1 split-K kernel geometry */
    QS_GEMM_PAIR_OFF = 2000,           /* the round-1 LDS-pair kernel never / ... */
    QS_GEMM_PAIR_FORCED = 2001,        /* ... always (where its preconditions hold) */
    QS_GEMM_TILED_OFF = 3000,          /* compute-bound kernels off */
    QS_GEMM_TILED_256 = 3001,          /* eight-wave 256-token tile forced */
    QS_GEMM_TILED_128 = 3002,          /* 128-token tile forced */
    QS_GEMM_WIDE_256 = 3003,           /* four-wave 256-token tile forced */
    QS_GEMM_TILED_DEBUG_BASE = 3100,   /* + bits: [QS_TIMING builds] parts of the tiled kernel off (sticky) */
    QS_GEMM_TILE_ORDER_BASE = 3200,    /* + 10 * persist_mode + order (sticky until QS_GEMM_TILE_ORDER_BASE) */
    QS_GEMM_ACT_FUSED = 3300,          /* qs_w4a8_*_gemm_silu_mul as one launch where it can [default] (sticky) */
    QS_GEMM_ACT_SPLIT = 3301,          /* ... always as two launches (sticky) */
    QS_GEMM_WIDE_DEBUG_BASE = 3400,    /* + bits: [QS_TIMING builds] parts of the wide kernel off (sticky) */
    QS_GEMM_RING_OFF = 4000,           /* decode ring kernel off (the round-1 kernels serve its shapes) */
    QS_GEMM_RING_NO_KSLICES = 4001,    /* ring kernel without K slices */
    QS_GEMM_RING_NO_GROUP_TERM = 4002, /* cost model without the per-group term */
    QS_GEMM_RING_NO_DOWN_OVERRIDE = 4003, /* without the measured <2,1> x 2 override for Llama-3's down_proj */
    QS_GEMM_RING_NO_MT8 = 4004,        /* without the 128-token geometry <8,2> */
    QS_GEMM_RING_GEOMETRY_BASE = 4100, /* + 100 * (k_slices - 1) + 10 * m_tiles + units: forced ring geometry */
    QS_GEMM_RING_GEOMETRY_END = 4500,
    QS_GEMM_PLANES_GEOMETRY_BASE = 4600, /* the same for the K-slice planes launches */
    QS_GEMM_PLANES_GEOMETRY_END = 5000,
    QS_GEMM_RING_FLAGS_BASE = 5000,    /* + bits (QS_RING_FLAG_*), sticky until QS_GEMM_RING_FLAGS_BASE */
    QS_GEMM_RING_FLAGS_END = 5000 + 16384
};
enum qs_ring_flag {                    /* qs_set_gemm_variant(QS_GEMM_RING_FLAGS_BASE + bits); results never change unless noted */
    QS_RING_FLAG_WEIGHTS_DEFAULT_POLICY = 1,  /* weight DMA without the non-temporal hint everywhere */
    QS_RING_FLAG_WEIGHTS_NT = 2,              /* ... non-temporal everywhere */
    QS_RING_FLAG_T_NO_REDUCTION = 4,          /* [QS_TIMING, wrong results] no cross-group reduction */
    QS_RING_FLAG_T_LEAVE_AFTER_LOOP = 8,      /* [QS_TIMING, wrong results] leave behind the k loop */
    QS_RING_FLAG_T_NO_MFMA = 32,              /* [QS_TIMING, wrong results] */
    QS_RING_FLAG_T_NO_OPERAND_READS = 64,     /* [QS_TIMING, wrong results] */
    QS_RING_FLAG_DEPTH_UNIT = 256,            /* * d: ring depth d = 3 .. 6 */
    QS_RING_FLAG_KSLICES_ONE_XCD = 4096,      /* K slices of a channel block on one XCD (the mapping of rounds 3-5) */
    QS_RING_FLAG_T_NO_LEVEL2 = 8192           /* [QS_TIMING, wrong results] per-group launches without the level-2 arithmetic */
};

/* Per-channel epilogue CONVENTION (process-wide; read at launch time by every per-channel W4A8 GEMM launch and by
 * qs_add_residual_rms_norm_general_planes, which finishes such a GEMM).  The reference statement
 *   (float(acc) * wscale) * ascale - w_sz * a_ssum          (w4a8_per_chn/gemm_cuda.cu:586-587)
 * is compiled there with nvcc's default --fmad=true, which may contract it; the CUDA binary cannot be produced here, so the
 * convention is selectable:  0 [default] = every operation rounded separately (the statement as written),
 *   1 = fmaf(float(acc) * wscale, ascale, -(w_sz * a_ssum)) - the fold of the last multiply into the subtraction that nvcc most
 *   plausibly performs (oracle/w4a8.py epilogue_per_chn(fma=True); differs on ~3.5e-4 of the outputs at Llama-3-8B shapes).
 * Returns QS_EINVAL for any other value.  Per-group GEMMs have no subtraction and are unaffected. */
int qs_set_gemm_epilogue(int convention);
int qs_get_gemm_epilogue(void);

/* Order of the per-token ROW SUM `a_ssums` written by qs_rms_norm_general (input_sum != NULL),
 * qs_add_residual_rms_norm_general and qs_add_residual_rms_norm_general_planes (process-wide; read at launch time).  It is the
 * value the per-channel GEMM epilogue multiplies by w_sz (w4a8_per_chn/gemm_cuda.cu:586).
 *   0 [default] = this library's order: fp32 chains per thread over 8-element chunks, wave butterfly, waves left to right;
 *   1 = the reference's own order (generalLayerNorm_fuse_sum, kernels/csrc/layernorm_kernels.cu:275-306): min(hidden, 1024)
 *       threads, thread t accumulates elements t, t + nt, ... in a HALF variable (one fp16 rounding per addition), partials
 *       all-reduced in fp32 by the 32-lane xor butterfly inside a warp and again over the warp slots
 *       (reduction_utils.cuh:25-30,68-85) - bit-equal to oracle/fused.py rms_norm_general(with_sum=True, sum_order="reference").
 * Int8 rows and scales do not depend on it.  invoke_quant_fuse_sum sums in fp32 in the reference too (fused_kernels.cu:104-122)
 * and has no second form.  Returns QS_EINVAL for any other value. */
int qs_set_row_sum_order(int order);
int qs_get_row_sum_order(void);

/* Measurement hook (no reference counterpart; SURVEY 8(d): "compute peak from the measured engine clock during the run").  While a
 * buffer is set, every launch of the compute-bound GEMM kernels (tiled / wide: M > 1024 or forced) with at most `workgroups`
 * workgroups makes workgroup b write buf[2 b] = its life in shader cycles (s_memtime) and buf[2 b + 1] = the same interval in
 * ticks of the constant 100 MHz counter (s_memrealtime): cycles / (ticks * 10 ns) = the engine clock that launch held under its own
 * load.  buf = device memory of 16 * workgroups bytes owned by the caller; (NULL, 0) stops it.  Results are unaffected. */
int qs_debug_gemm_clock_probe(void* buf, int workgroups);

/* Plan only: the W4A8 GEMM dispatcher's kernel choice for an (M, N, K) problem - the same planning function the launches
 * use, without touching the device - in plan5 = {family, p0, p1, p2, p3}: family 1 = split-K kernel (m_tiles, waves,
 * cross-block slices, xcd mapping), 2 = LDS-pair kernel, 3 = ring kernel (m_tiles, units, token blocks, K slices; K slices
 * assume the split-K workspace, without which a launch runs un-split), 4 = tiled kernel (8 = 256-token tile, 4 = 128-token
 * tile), 5 = four-wave tiled kernel (8); all zero for M = 0.  No reference counterpart: it makes the selection heuristics testable on a CPU-only machine
 * (tests/test_dispatch_plan.py).  per_group: 0 = per-channel, 1 = per-group-128.  Honours qs_set_gemm_variant. */
int qs_w4a8_gemm_plan(int per_group, int M, int N, int K, int* plan5);

/* ------------------------------------------------------------------------------------------------------------
 * Decode attention over the paged, quantised KV cache.
 * Replaces qserve_backend.fused_attention.single_query_attention
 *   (kernels/csrc/fused_attention/fused_attention.h:13-28, fused_attention.cpp:150-240).
 *   q   half [B,H,Dh]   view, element strides (q_stride0, Dh, 1)
 *   k,v half [B,Hkv,Dh] views, element strides (kv_stride0, Dh, 1)          (un-rotated new token)
 *   kv_pointers int64 [B,2,max_blocks]: device ADDRESSES of K pages ([:,0,:]) and V pages ([:,1,:])
 *   length_per_sample int32 [B]: context length INCLUDING the new token, i.e. the new token sits at position
 *                     length-1 and attends to length-1 cached tokens.  May be NULL: then, exactly as in the reference
 *                     (decoderMaskedMultiheadAttentionTemplate.hpp:901, tlength = length_per_sample ?
 *                     length_per_sample[bi]-1 : timestep), every sequence has `timestep` CACHED tokens and the new token
 *                     is written at position `timestep`
 *   out half [B,H,Dh] contiguous (the reference returns torch::empty_like(q))
 * Layout contract (QS_EINVAL otherwise, checked before any device call): q, k, v and out 16-byte aligned; q_stride0 and
 * kv_stride0 multiples of 8 elements, q_stride0 >= H*Dh, kv_stride0 >= Hkv*Dh.  Any such stride is served (padded rows, views
 * into wider buffers, k and v in buffers of their own) - but k and v share ONE token stride.
 * Page layout (kvCacheUtils.h:47-126): [Hkv][tokens_per_block][Dh'] data, then half scale[Hkv][tpb], then
 * half zero[Hkv][tpb]; Dh' = size_per_token / Hkv bytes.
 * Side effect: quantises the new token's rotated K and V into the page of position length-1.
 * Supported (what the reference instantiates): Dh = 128, tokens_per_block = 64, kv_cache_with_zeros.
 * neox_rotary_style is accepted and has no effect: the reference never forwards it (fused_attention.cpp:109 is commented out;
 * update_kv_cache.cu:57 hard-codes kROPE_GPT_NEOX) - RoPE is always the NeoX pairing (d, d + 64).  Likewise the op-level
 * `alibi_slopes` argument is checked and dropped by the reference (fused_attention.cpp:91,193-199) and by both mirrors here.
 * ---------------------------------------------------------------------------------------------------------- */
int qs_single_query_attention(const void* q, const void* k, const void* v, const int64_t* kv_pointers,
                              const int32_t* length_per_sample, void* out, int batch, int num_heads,
                              int num_kv_heads, int head_dim, int64_t q_stride0, int64_t kv_stride0,
                              int max_blocks, int memory_max_seqlen, int tokens_per_block, int size_per_token,
                              int timestep, int rotary_embedding_dim, float rotary_base, int neox_rotary_style,
                              int int4_kv_cache, int kv_cache_with_zeros, qs_stream_t stream);

/* Pair fusion for the decode loop (no reference counterpart): single_query_attention followed by
 * invoke_quant(_fuse_sum) of its output (llama_w4a8_unpad.py:253-282) as ONE call.  `out` receives the fp16 attention
 * output exactly as above; quant_out int8 [B, H*Dh], quant_scale half [B], quant_sum half [B] (may be NULL) receive what
 * qs_invoke_quant(quant_out, out, quant_sum, quant_scale, B, H*Dh) would write - BIT-IDENTICAL.  Where the chosen
 * attention kernel can finish the row itself (matrix-core KV4 kernel, no KV split, H*Dh <= 4096) this is one launch,
 * otherwise the two launches are issued here.  Uses the per-device arrival-counter scratch (same stream rule as above). */
int qs_single_query_attention_quant(const void* q, const void* k, const void* v, const int64_t* kv_pointers,
                                    const int32_t* length_per_sample, void* out, int8_t* quant_out, void* quant_sum,
                                    void* quant_scale, int batch, int num_heads, int num_kv_heads, int head_dim,
                                    int64_t q_stride0, int64_t kv_stride0, int max_blocks, int memory_max_seqlen,
                                    int tokens_per_block, int size_per_token, int timestep, int rotary_embedding_dim,
                                    float rotary_base, int neox_rotary_style, int int4_kv_cache, int kv_cache_with_zeros,
                                    qs_stream_t stream);

/* Kernel selection for A/B tests: 0 = matrix-core kernels (KV4 and KV8) with the split-KV heuristic [default],
 * 1 = VALU kernels, 2 = prefill writer without the RoPE table, 3 = KV4 matrix-core kernel with the service wave always
 * owning pages (A/B of the page-ownership rule), 5 = one raw barrier instead of the polled operand flag, 7 = the attention +
 * quant fusion hands the PAYLOAD to the last KV head's workgroup also where it otherwise gathers the row statistics (group sizes
 * 4 and 8; A/B of the hand-over, same bits), 100 + n = matrix-core kernels with exactly n KV splits.
 * (200 + bits: ablation / trace instantiations of the KV4 kernel, QS_TIMING builds only; ignored by the shipped library.) */
void qs_set_attention_variant(int variant);

/* Plan only (no device access, CPU-testable like qs_w4a8_gemm_plan): which decode attention kernel the dispatcher's planning
 * function takes for (batch, heads, kv heads, page-table width, longest context) and how it splits the context:
 * plan3 = {family, kv_splits, waves per workgroup}; family 1 = matrix-core KV4 kernel, 2 = matrix-core KV8 kernel,
 * 3 = VALU kernel (page tables wider than 192 entries, or forced by qs_set_attention_variant(1)).  kv_splits is the plan;
 * a launch runs fewer where the split workspace cannot hold them.  All zero for batch = 0. */
int qs_attention_plan(int batch, int num_heads, int num_kv_heads, int max_blocks, int timestep, int int4_kv_cache,
                      int* plan3);

/* Prefill KV writer.  Replaces qserve_backend.fused_attention.apply_bias_rope_update_kv_cache
 *   (kernels/csrc/fused_attention/update_kv_cache.h:11-27, update_kv_cache.cu:20-108).
 *   qkv half [num_tokens, (H+2Hkv)*Dh] modified in place (rotated q and k are written back);
 *   seq_lens int32 [batch]; padding_offset int32 [num_tokens]; kv_pointers as above (NULL: no cache write). */
int qs_apply_bias_rope_update_kv_cache(void* qkv, const int32_t* seq_lens, const int32_t* padding_offset,
                                       const int64_t* kv_pointers, int num_tokens, int batch, int max_blocks,
                                       int head_num, int kv_head_num, int seq_len, int tokens_per_block,
                                       int size_per_token, int rotary_embedding_dim, float rotary_embedding_base,
                                       int rotary_embedding_max_positions, int neox_rotary_style,
                                       int int4_kv_cache, int kv_cache_with_zeros, qs_stream_t stream);

/* Replaces qserve_backend.fused_attention.compute_padding_offsets (input_metadata_helper.h:12-13). */
int qs_compute_padding_offsets(int32_t* padding_offsets, const int32_t* cu_seqlens, int batch, int max_seqlen,
                               qs_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Activation-side kernels adjacent to the hot path (they produce the GEMM's A / ascales / a_ssums).
 * Replace qserve_backend.fused_kernels.invoke_quant(_fuse_sum)      (kernels/csrc/fused.cpp:47-71),
 *         qserve_backend.layernorm_ops.rms_norm(_general(_fuse_sum)) (kernels/csrc/layernorm.cpp:47-72),
 *         qserve_backend.activation_ops.silu_and_mul                 (kernels/csrc/activation.cpp:25-39).
 * hidden % 8 == 0 required.  `input_sum` may be NULL (non-_fuse_sum variants).
 * ---------------------------------------------------------------------------------------------------------- */
int qs_invoke_quant(int8_t* out, const void* input, void* input_sum, void* scale, int num_tokens, int hidden,
                    qs_stream_t stream);
int qs_rms_norm_general(int8_t* out, const void* input, const void* weight, void* input_sum, void* scaling,
                        float epsilon, int num_tokens, int hidden, qs_stream_t stream);
int qs_rms_norm(void* out, const void* input, const void* weight, float epsilon, int num_tokens, int hidden,
                qs_stream_t stream);
int qs_silu_and_mul(void* out, const void* input, int num_tokens, int d, qs_stream_t stream);
/* fp16 residual add (the reference does this with a torch add, llama_w4a8_unpad.py:348,360): a += b */
int qs_residual_add(void* a, const void* b, int64_t numel, qs_stream_t stream);
/* greedy sampling helper (the reference's sampler is torch: argmax over the fp16 logits, layers/sampler.py): out[r] = index
 * of the first maximum of row r of x (fp16 [rows, n], row stride in elements, 16-byte aligned rows; NaN-free). */
int qs_argmax_rows(const void* x, int64_t* out, int rows, int n, int64_t row_stride, qs_stream_t stream);
/* A/B and tests: -1 = heuristic (few long rows are split over up to 8 workgroups per row, candidates meeting in a
 * device-scope atomic max; needs a library-owned 96 KiB scratch that is never allocated during stream capture),
 * 1 = one workgroup per row, >= 2 = forced split. */
void qs_debug_argmax_split(int split);

/* Pair fusions for the decode loop (no reference counterpart; each is BIT-IDENTICAL to the two calls it replaces and
 * exists because at decode batch sizes every one of these row kernels is a fixed ~5 us latency chain):
 *   qs_add_residual_rms_norm_general == qs_residual_add(hidden_io, delta) ; qs_rms_norm_general(out, hidden_io, ...)
 *        (llama_w4a8_unpad.py:348-351 / :360 + next layer's :337 - the torch add followed by the layer norm)
 *   qs_silu_and_mul_quant            == qs_silu_and_mul(tmp, input) ; qs_invoke_quant(out, tmp, ...)
 *        (llama_w4a8_unpad.py:84-91: act_fn then invoke_quant(_fuse_sum)); `input_sum` may be NULL as above. */
int qs_add_residual_rms_norm_general(int8_t* out, void* hidden_io, const void* delta, const void* weight,
                                     void* input_sum, void* scaling, float epsilon, int num_tokens, int hidden,
                                     qs_stream_t stream);
/*   == qs_w4a8_*_gemm(in, kernel, ..., delta) ; qs_add_residual_rms_norm_general(out, hidden_io, delta, ...) where the GEMM ran as
 *   qs_w4a8_*_gemm_planes: delta[t][n] = fp16(epilogue(sum over the k_slices planes)) is formed inside the row kernel.
 *   wscales / w_szs fp16 [hidden] and ascales / a_ssums fp16 [num_tokens] are the GEMM's epilogue operands (w_szs and a_ssums
 *   NULL together = per-group epilogue); ascales / a_ssums MAY alias scaling / input_sum (a row reads its own values first).
 *   plane_stride = elements between planes (>= num_tokens * hidden); hidden <= 4096. */
int qs_add_residual_rms_norm_general_planes(int8_t* out, void* hidden_io, const int32_t* planes, int k_slices,
                                            int64_t plane_stride, const void* wscales, const void* w_szs, const void* ascales,
                                            const void* a_ssums, const void* weight, void* input_sum, void* scaling,
                                            float epsilon, int num_tokens, int hidden, qs_stream_t stream);
int qs_silu_and_mul_quant(int8_t* out, const void* input, void* input_sum, void* scale, int num_tokens, int d,
                          qs_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Prefill attention: provider for the call the reference makes into the un-vendored flash-attn wheel,
 *   flash_attn.flash_attn_interface.flash_attn_varlen_func(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q,
 *   max_seqlen_k, dropout_p=0, softmax_scale=None, causal=True)      (llama_w4a8_unpad.py:30,232-242).
 *   q   half [total_q, H, 128]   token stride q_stride0 elements (views into the packed qkv buffer are fine)
 *   k,v half [total_k, Hkv, 128] token strides k_stride0 / v_stride0
 *   out half [total_q, H, 128]   token stride o_stride0
 *   cu_seqlens_q / cu_seqlens_k int32 [batch+1] (device).  causal: bottom-right aligned when lengths differ (v2.1+).
 * head_dim must be 128; dropout, ALiBi, sliding windows and returning probabilities are not provided.
 * Layout contract (QS_EINVAL otherwise, checked before any device call): heads contiguous (element strides (stride0, 128, 1));
 *   q, k, v   16-byte aligned; q_stride0, k_stride0, v_stride0 multiples of 8 elements, >= the token's heads (H*128 resp.
 *             Hkv*128) and < 2^24.  q, k and v may live in three buffers with three strides.  Every such stride is served with the
 *             same bits; K strides that are multiples of 128 elements (whole heads per token: packed qkv, contiguous k) take the
 *             one-register tile offsets of the key loop, all others its general per-piece offsets;
 *   out       8-byte aligned, o_stride0 a multiple of 4 elements, >= H*128 and < 2^24; rows are written 16 bytes at a time where
 *             out is 16-byte aligned and o_stride0 a multiple of 8, 8 bytes at a time otherwise.  Nothing outside the rows'
 *             H*128 elements is written.
 * ---------------------------------------------------------------------------------------------------------- */
int qs_flash_attn_varlen_fwd(const void* q, const void* k, const void* v, void* out, const int32_t* cu_seqlens_q,
                             const int32_t* cu_seqlens_k, int batch, int num_heads, int num_kv_heads, int head_dim,
                             int64_t q_stride0, int64_t k_stride0, int64_t v_stride0, int64_t o_stride0,
                             int max_seqlen_q, int max_seqlen_k, float softmax_scale, int causal, qs_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Direct-access fp16 sum all-reduce for the tensor-parallel step (no reference counterpart: the reference's
 * tensor parallelism is inert).  Every rank owns one uncached buffer pair (input | output) that all peers map through
 * HIP IPC; one kernel per call: flag exchange, each rank reduces its slice straight out of the peers' inputs (fp32, rank
 * order, one rounding) and writes it straight into everybody's output, flag exchange.  A kernel on the caller's stream
 * like any other: capturable in a hipGraph.  All waits are bounded (qs_comm_error reports a timeout).  UNMEASURED on
 * multi-GPU hardware; torch.distributed / RCCL stays the default of qserve_amd.tp.all_reduce_sum_.
 *   qs_comm_create        allocates this rank's region (current device), returns the communicator and a 64-byte IPC handle
 *   qs_comm_connect       handles = world x 64 bytes in rank order (gathered by the caller, e.g. all_gather_object)
 *   qs_comm_connect_local same-process ranks: the other communicators themselves, no IPC (tests)
 *   qs_comm_input/output  device pointers: the rank's addend is written to input (e.g. as the row-parallel GEMM's output
 *                         buffer), the sum over all ranks is in output once qs_comm_all_reduce_f16's kernel has retired
 *   numel % (8 * world) == 0, numel * 2 <= payload_bytes.  After a time-out the ranks' device-side epochs no longer
 *   match: destroy and re-create the communicators. */
int qs_comm_create(int rank, int world, int64_t payload_bytes, void** comm_out, void* ipc_handle64);
int qs_comm_connect(void* comm, const void* handles);
int qs_comm_connect_local(void* comm, void* const* peer_comms);
void* qs_comm_input(void* comm);
void* qs_comm_output(void* comm);
int qs_comm_all_reduce_f16(void* comm, int64_t numel, qs_stream_t stream);
/* tests: the calls of all ranks of a same-process group (qs_comm_connect_local) as ONE dispatch */
int qs_comm_all_reduce_f16_group(void* const* comms, int world, int64_t numel, qs_stream_t stream);
int qs_comm_error(void* comm);
int qs_comm_destroy(void* comm);

/* ------------------------------------------------------------------------------------------------------------
 * Bounded in-launch waits (no reference counterpart).  Two launches of this library contain a cross-workgroup hand-off that
 * polls inside the launch: the K-slice seam of the decode W4A8 GEMMs and the finisher of qs_single_query_attention_quant.  They
 * rely on in-order workgroup dispatch and on one-stream-at-a-time use of a scratch set (see the header comment).  Every such
 * wait is BOUNDED: after ~1e6 polls (seconds) the waiting wave gives up, sets a bit in the error word of its scratch set and finishes
 * the launch with what it has - results of that launch are invalid, the GPU is not hung.
 *   qs_device_status   error_bits = OR of 1 (K-slice seam gave up), 2 (attention + quant hand-over gave up) on the CURRENT
 *                      device since the last reset; blocking (a device-to-host copy behind the work launched so far) - call it
 *                      at checkpoints, not per launch.  Returns QS_OK when the word could be read; a non-zero word also sets
 *                      qs_last_error().
 *   qs_device_reset    synchronises the device, clears the word and puts the hand-off scratch back into its initial state
 *                      (K-slice slabs sentinel-filled, exchange rows / generation words zeroed).  Required after a non-zero
 *                      status and after an aborted launch before the library is used again; replayed hipGraphs stay valid
 *                      (no address changes).
 *   qs_debug_inject_fault  tests only: arms a ONE-SHOT fault - bit 0: the next K-sliced ring GEMM launch, bit 1: the next
 *                      fused attention + quant launch runs with one producer that never delivers (and a short poll bound), so
 *                      that the give-up path, the status word and the recovery can be exercised.  The results of THAT launch
 *                      are wrong by design; 0 disarms. */
int qs_device_status(int* error_bits);
int qs_device_reset(void);
int qs_debug_inject_fault(int what);

/* Per-stream scratch (no reference counterpart; the reference's engine is single-stream).  By default every stream of a device
 * shares ONE set of the library's scratch areas, so scratch-using launches must not overlap across streams.  A caller that runs
 * the library on several streams of one device concurrently binds the extra streams first:
 *   qs_stream_scratch_bind    gives `stream` (on the calling thread's current device) its own split-K / K-slice slabs, split-KV
 *                             partials, hand-over rows and argmax keys (~130 MiB, allocated HERE - call it outside stream capture,
 *                             before the stream's first launch or capture; idempotent).  Launches issued or captured on the stream
 *                             use these areas from then on; qs_device_status / qs_device_reset cover every bound stream.
 *                             QS_ENOSUP when the device's 7 slots are taken, QS_EINVAL while the stream is capturing.
 *   qs_stream_scratch_unbind  forgets the binding (the stream falls back to the shared areas); the slot's memory is kept and
 *                             handed to the next bind on this device, so graphs captured on the stream stay valid - but they
 *                             then share the areas with that next stream. */
int qs_stream_scratch_bind(qs_stream_t stream);
int qs_stream_scratch_unbind(qs_stream_t stream);

/* Device self-test (tests/test_fused_gpu.py): the DPP / permlane wave reductions every row kernel uses round exactly like
 * the shuffle butterfly they replace.  in: float [n] (n % 64 == 0); out: float [n/64][4] = {sum, sum by shuffles, max, max
 * by shuffles} per 64-value block. */
int qs_debug_wave_reduce_selftest(const float* in, float* out, int n, qs_stream_t stream);

/* A/B hook of the prefill attention provider (process-wide, see qs_set_gemm_variant): 0 [default] = the round-6 kernel (Q fragments
 * complete before the key loop, no accumulator copies in it, lazy running maximum, whole-row output through LDS); 1 = the
 * kernel of rounds 2-5.  Both compute the same softmax within the provider's tolerance (tests/test_flash_gpu.py runs both).
 * QS_EINVAL for any other value. */
int qs_debug_flash_variant(int variant);

/* Append attention (no reference counterpart): n >= 1 NEW tokens per sequence against a context that already sits in the quantised
 * pages - chunked prefill, prefix reuse, verification of drafted tokens.  Sequence b has past_lens[b] tokens in its pages and
 * n = cu_seqlens_q[b + 1] - cu_seqlens_q[b] new rows in the packed fp16 qkv buffer [T, (H + 2 Hkv) * 128] (n = 0 is legal);
 * past + n <= 64 * max_blocks, past need not be a multiple of 64.  Device pointers: cu_seqlens_q int32 [batch + 1], past_lens
 * int32 [batch], kv_pointers int64 [batch, 2, max_blocks] (page addresses, as for qs_single_query_attention).
 *   qs_append_rope_update_kv_cache  new token i: q and k NeoX-rotated at position past + i in place in qkv; rotated K and raw V
 *                      quantised per (token, KV head) into the page slot of position past + i - byte for byte what
 *                      qs_apply_bias_rope_update_kv_cache stores for that position.
 *   qs_append_attention  query row i attends to keys 0 .. past + i: positions < past de-quantised from the pages (the decode
 *                      kernels' values), positions >= past in fp16 from the ALREADY ROTATED qkv (rotated k, raw v).  fp32 softmax,
 *                      scale 1/sqrt(128), out fp16 [T, H, 128] with row stride out_stride0 (elements).  The two calls touch
 *                      disjoint page slots: no ordering is needed between them.  past = 0 is the prefill attention, n = 1 the
 *                      decode attention.  Layout contract (QS_EINVAL otherwise, checked before any device call): qkv and out
 *                      16-byte aligned; qkv_stride0 a multiple of 8 elements, >= (H + 2 Hkv) * 128 and < 2^24; out_stride0 a
 *                      multiple of 8, >= H * 128.  Every such stride is served with the same bits (padded rows, views into
 *                      wider buffers); nothing outside the rows' H * 128 elements is written.
 *   qs_append_attention_plan  pure (no device access): plan3 = {tokens per query tile, query tiles per sequence at max_seqlen_q,
 *                      waves per workgroup} of the launch the arguments would get; all zero for an empty launch.  One workgroup
 *                      serves a query tile of ONE KV head with all H / Hkv query heads: rows = (token, head-in-group) pairs.
 *   qs_append_attention_split  the same attention (same arguments, layout contract and validation, checked before any device
 *                      call) with the past of every sequence cut into up to num_splits contiguous page ranges that run as workgroups
 *                      of their own - for long contexts at small batch, where the un-split launch leaves most of the chip idle.  Two
 *                      launches on `stream`: the split kernel leaves per-row partial records (un-normalised fp32 O[128], running
 *                      maximum, sum) in the library's split-KV workspace, a merge kernel combines them in fp32 and stores fp16 through
 *                      out_stride0; nothing outside the rows' H * 128 elements is written.  The ranges are computed on the device
 *                      from past_lens: max_past is an upper-bound HINT for the planner only (negative = 64 * max_blocks), never
 *                      something a result depends on.  num_splits = 0 asks qs_append_attention_split_plan with max_past;
 *                      num_splits >= 1 forces that count (tests, sweeps), clamped to 64 and to what the workspace holds;
 *                      num_splits < 0 is QS_EINVAL.  An effective count of 1 - and a call that cannot have the workspace (too
 *                      large, or its first use falls inside a stream capture) - runs qs_append_attention's launch: bit-identical to it.
 *   qs_append_attention_split_plan  pure (no device access, deterministic in its arguments): plan5 = {tokens per query tile, query
 *                      tiles, waves per workgroup [the three of qs_append_attention_plan], splits >= 1, KiB of workspace the partial
 *                      records take (0 with one split)}; all zero for an empty launch.  max_past < 0 is QS_EINVAL.
 *   qs_append_attention_shared  the same attention - by definition what qs_append_attention gives on the same arguments - for a
 *                      batch cut into num_groups GROUPS of batch-adjacent sequences whose members hold the same leading pages
 *                      (prefix reuse: a system prompt, a few-shot header).  Device arrays: group_offsets int32 [num_groups + 1] (group g
 *                      is sequences group_offsets[g] .. group_offsets[g + 1] - 1; the groups partition 0 .. batch - 1), prefix_lens
 *                      int32 [num_groups], seq_group int32 [batch] (the group of every sequence, non-decreasing).  prefix_lens[g] is
 *                      the number of leading cached tokens every member of group g has in common.  PRECONDITIONS, kept by the
 *                      caller: it is a multiple of 64 (whole pages), at most past_lens[b] of every member b, and entry p of a
 *                      member's K table and of its V table EQUALS the first member's for every p < prefix_lens[g] / 64.  A prefix
 *                      of 0, a group of one sequence, members with n = 0 and members whose past equals the prefix are legal.
 *                      Sharing changes who reads the bytes, never a value beyond fp32 summation order: with P >= 1 prefix splits in
 *                      effect the prefix pages are read ONCE per group, THROUGH THE FIRST MEMBER'S TABLE ONLY, for all the group's
 *                      new rows (max_group_tokens: an upper bound of a group's new tokens, as max_seqlen_q is of a sequence's), each
 *                      sequence's pages behind the prefix and its new tokens as in qs_append_attention_split; partial records go to
 *                      the split-KV workspace (same allocation rule, not enlarged) and a merge launch joins them: two launches on
 *                      `stream`, nothing outside the rows' H * 128 elements is written, no page is written.  The equal-entries
 *                      precondition is also what makes the fall-backs correct: without the workspace (its first use inside a stream
 *                      capture) the entry runs qs_append_attention, and "do not share" runs qs_append_attention_split over the whole
 *                      past - both read every member's own table.  On a violated precondition no address outside the tables and the
 *                      pages they name is formed: the device rounds a prefix down to whole pages and cuts it to 64 * max_blocks, group
 *                      bounds and indices are cut to the batch; a member whose past is shorter than the prefix gets unspecified rows
 *                      and nothing else is affected.  max_prefix / max_suffix_past: upper-bound HINTS (of prefix_lens, and of
 *                      past_lens[b] - prefix) for the planner only, negative = 64 * max_blocks, never something a result depends on.
 *                      num_prefix_splits / num_suffix_splits: 0 asks qs_append_shared_plan, >= 1 forces that count (clamped to 64 and
 *                      to what the workspace holds); num_prefix_splits = -1 forces "do not share".  Validation as for
 *                      qs_append_attention, and QS_EINVAL for a null group array, num_groups outside 1 .. batch, a negative count,
 *                      num_prefix_splits < -1 or num_suffix_splits < 0 - before any device call.  batch, num_tokens, max_seqlen_q or
 *                      max_group_tokens of 0: QS_OK without a launch.
 *   qs_append_shared_plan  pure (no device access, deterministic in its arguments): plan8 = {tokens per query tile, query tiles per
 *                      sequence, waves per workgroup [the three of qs_append_attention_plan], suffix splits S, query tiles per group
 *                      at max_group_tokens, prefix splits P, record waves (suffix | prefix << 8: the waves of a workgroup that can own
 *                      a row - a record block exists only for those), KiB of workspace (rounded up)}; all zero for an empty launch.
 *                      P = 0 means "do not share" - num_groups == batch, max_prefix < 64, or no room in the workspace: S and the KiB
 *                      are then qs_append_attention_split_plan's for max_prefix + max_suffix_past, the record waves 4.
 * QS_EINVAL: null pointers, bad sizes / head counts / strides;  QS_ENOSUP: head_dim != 128, tokens_per_block != 64, caches
 * without zero points, H / Hkv > 8.
 *
 * Tree-draft verification (Medusa / EAGLE / SpecInfer style: several candidates per position, verified in one pass).  The n <= 64 new
 * rows of a sequence are the NODES OF A TREE IN TOPOLOGICAL ORDER (a parent's index is below its child's).  tree_mask: device uint64
 * [T], 8-byte aligned, one word per row of qkv; bit j of node i's word = "node i sees new token j of its own sequence", bits >= n are
 * ignored.  A well-formed word is ancestor-closed and has its own bit set (a chain: (2 << i) - 1); the depth of a node is
 * popcount(word) - 1 - the one source of truth, there is no depth array.
 *   qs_append_tree_rope_update_kv_cache  qs_append_rope_update_kv_cache with two positions per node: q and k are NeoX-rotated at
 *                      position past + depth (an empty word: depth 0), the rotated K and raw V are quantised into the slot of
 *                      position past + i.  Same arithmetic per element, same cos / sin, slots beyond the pointer table are skipped;
 *                      with chain words it leaves qs_append_rope_update_kv_cache's bytes.  qkv 16-byte aligned.
 *   qs_append_tree_attention  qs_append_attention_split (same arguments - max_past and num_splits included -, layout contract,
 *                      validation, workspace, merge and fall-back rules; num_splits = 1 runs un-split) with another rule among the new
 *                      tokens: row i sees every cached key < past, and new key j iff j < n and bit j of its word is set.  Nothing else
 *                      is assumed - no j <= i, no closure.  A row that sees no key is exactly 0.  Softmax, scale and de-quantised
 *                      values are unchanged: with chain words the result is bit-identical to the linear entries.  max_seqlen_q > 64
 *                      is QS_EINVAL before any device call.
 *   qs_kv_cache_commit_path  after acceptance: for k < accept_lens[b], slot past + k of sequence b receives the bytes (data, fp16
 *                      scale, fp16 zero; K and V, every KV head) of slot past + accept_idx[b, k].  accept_idx int32 [batch, max_accept]
 *                      with strictly increasing rows (hence accept_idx[b, k] >= k) of node indices 0 .. 63, accept_lens int32 [batch],
 *                      max_accept <= 64 (QS_EINVAL otherwise).  Every source is read before any destination is written (a source may
 *                      be another move's destination; moves cross page boundaries); identity moves are skipped; no other byte of any
 *                      page changes.  Slots >= past + accept_lens[b] KEEP WHAT THEY HOLD - the rejected nodes' stale K / V -, which every
 *                      reader masks by the sequence length and the next writer overwrites.  The caller advances its lengths.
 *   qs_tree_accept_greedy  the greedy walk over the verified tree, on the device (nothing is read back).  tokens / argmax: int64 [T], 8-byte
 *                      aligned - the token every node carries and the model's arg-max at every node; parents: int32 [T], an index INTO THE
 *                      NODE'S OWN SEQUENCE, -1 = hangs off the context; sequence b has n = cu_seqlens_q[b + 1] - cu_seqlens_q[b] nodes, cut
 *                      to 64.  If n >= 1 node 0 is accepted; from the current node cur the next one is the LOWEST c with cur < c < n,
 *                      parents[c] == cur and tokens[c] == argmax[cur]; the walk ends when there is none or the path holds max_accept
 *                      (1 .. 64) nodes.  accept_idx int32 [batch, max_accept]: the path, 0 behind it; accept_lens int32 [batch]: its length;
 *                      last_row int64 [batch] (may be null): cu_seqlens_q[b] + the last accepted node, the global row; next_token int64
 *                      [batch] (may be null): argmax[last_row[b]].  n = 0: length 0, last_row -1, next_token[b] NOT written.  Only c > cur is
 *                      a candidate, so the walk increases strictly whatever parents holds (p >= i, p < -1, self-loops): it ends within n
 *                      levels and reads nothing outside the sequence's rows.  QS_EINVAL before any device call: a null required pointer,
 *                      negative sizes, max_accept outside 1 .. 64, a misaligned 8-byte array.  batch or num_tokens of 0: QS_OK, no launch.
 *   qs_kv_cache_commit_path_layers  qs_kv_cache_commit_path for every layer in ONE launch.  layer_tables: device int64 [num_layers], 8-byte
 *                      aligned, entry l = the device address of layer l's kv_pointers [batch, 2, max_blocks]; past_lens, accept_idx and
 *                      accept_lens are common to the layers.  Per (layer, K | V, KV head, sequence) the rule is qs_kv_cache_commit_path's,
 *                      word for word - the pages end byte-identical to num_layers calls of it.  Validation as there, plus num_layers >= 1. */
int qs_append_rope_update_kv_cache(void* qkv, const int32_t* cu_seqlens_q, const int32_t* past_lens,
                                   const int64_t* kv_pointers, int num_tokens, int batch, int max_blocks, int head_num,
                                   int kv_head_num, int tokens_per_block, int size_per_token, int rotary_embedding_dim,
                                   float rotary_base, int int4_kv_cache, int kv_cache_with_zeros, qs_stream_t stream);
int qs_append_attention(const void* qkv, void* out, const int32_t* cu_seqlens_q, const int32_t* past_lens,
                        const int64_t* kv_pointers, int num_tokens, int batch, int max_seqlen_q, int max_blocks, int num_heads,
                        int num_kv_heads, int head_dim, int64_t qkv_stride0, int64_t out_stride0, int tokens_per_block,
                        int size_per_token, int int4_kv_cache, int kv_cache_with_zeros, qs_stream_t stream);
int qs_append_attention_plan(int batch, int max_seqlen_q, int num_heads, int num_kv_heads, int* plan3);
int qs_append_attention_split(const void* qkv, void* out, const int32_t* cu_seqlens_q, const int32_t* past_lens,
                              const int64_t* kv_pointers, int num_tokens, int batch, int max_seqlen_q, int max_blocks, int num_heads,
                              int num_kv_heads, int head_dim, int64_t qkv_stride0, int64_t out_stride0, int tokens_per_block,
                              int size_per_token, int int4_kv_cache, int kv_cache_with_zeros, int max_past, int num_splits,
                              qs_stream_t stream);
int qs_append_attention_split_plan(int batch, int max_seqlen_q, int max_past, int num_heads, int num_kv_heads, int int4_kv_cache,
                                   int* plan5);
int qs_append_attention_shared(const void* qkv, void* out, const int32_t* cu_seqlens_q, const int32_t* past_lens,
                               const int64_t* kv_pointers, const int32_t* group_offsets, const int32_t* prefix_lens,
                               const int32_t* seq_group, int num_tokens, int batch, int num_groups, int max_seqlen_q,
                               int max_group_tokens, int max_blocks, int num_heads, int num_kv_heads, int head_dim, int64_t qkv_stride0,
                               int64_t out_stride0, int tokens_per_block, int size_per_token, int int4_kv_cache, int kv_cache_with_zeros,
                               int max_prefix, int max_suffix_past, int num_prefix_splits, int num_suffix_splits, qs_stream_t stream);
int qs_append_shared_plan(int batch, int max_seqlen_q, int num_groups, int max_group_tokens, int max_prefix, int max_suffix_past,
                          int num_heads, int num_kv_heads, int int4_kv_cache, int* plan8);
int qs_append_tree_rope_update_kv_cache(void* qkv, const int32_t* cu_seqlens_q, const int32_t* past_lens,
                                        const int64_t* kv_pointers, const uint64_t* tree_mask, int num_tokens, int batch,
                                        int max_blocks, int head_num, int kv_head_num, int tokens_per_block, int size_per_token,
                                        int rotary_embedding_dim, float rotary_base, int int4_kv_cache, int kv_cache_with_zeros,
                                        qs_stream_t stream);
int qs_append_tree_attention(const void* qkv, void* out, const int32_t* cu_seqlens_q, const int32_t* past_lens,
                             const int64_t* kv_pointers, const uint64_t* tree_mask, int num_tokens, int batch, int max_seqlen_q,
                             int max_blocks, int num_heads, int num_kv_heads, int head_dim, int64_t qkv_stride0, int64_t out_stride0,
                             int tokens_per_block, int size_per_token, int int4_kv_cache, int kv_cache_with_zeros, int max_past,
                             int num_splits, qs_stream_t stream);
int qs_kv_cache_commit_path(const int64_t* kv_pointers, const int32_t* past_lens, const int32_t* accept_idx,
                            const int32_t* accept_lens, int batch, int max_accept, int max_blocks, int kv_head_num,
                            int tokens_per_block, int size_per_token, int int4_kv_cache, int kv_cache_with_zeros, qs_stream_t stream);
int qs_tree_accept_greedy(const int64_t* tokens, const int64_t* argmax, const int32_t* parents, const int32_t* cu_seqlens_q,
                          int num_tokens, int batch, int max_accept, int32_t* accept_idx, int32_t* accept_lens, int64_t* last_row,
                          int64_t* next_token, qs_stream_t stream);
int qs_kv_cache_commit_path_layers(const int64_t* layer_tables, int num_layers, const int32_t* past_lens, const int32_t* accept_idx,
                                   const int32_t* accept_lens, int batch, int max_accept, int max_blocks, int kv_head_num,
                                   int tokens_per_block, int size_per_token, int int4_kv_cache, int kv_cache_with_zeros,
                                   qs_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Row sampler (no reference counterpart: the reference's sampler layer applies its logits warpers and draws with torch ops,
 * qserve/modeling/layers/sampler.py).  One token per row of fp16 logits [rows, row_stride] under temperature, top-k and top-p, on the
 * device: capturable, nothing allocated, nothing read back, no hidden state.  temperature / top_k / top_p apply where the per-row
 * device array (row_temperature / row_top_p float [rows], row_top_k int32 [rows]) is null.
 *
 * Per row, in exact arithmetic (x_i the fp16 logit, T, k, p the row's parameters, m = max x, w_i = exp((x_i - m) / T), W = sum w):
 *   greedy     T < 1e-5 or p < 1e-8 (the reference's greedy conditions): out = the first index of the maximum (qs_argmax_rows).
 *   nucleus    tau_p = the largest logit VALUE v with sum_{x_i >= v} w_i >= p * W; p >= 1: off.  The cut is at the granularity of values:
 *              every token tied at the threshold stays (a sort-based sampler cuts inside a tie class, by sort order).
 *   top-k      tau_k = the k-th largest logit; ties at it stay; k <= 0 or k >= n: off.
 *   order      the nucleus is taken on the full tempered distribution, then intersected with top-k (the reference's warper order):
 *              S = {i : x_i >= max(tau_p, tau_k)}, W_S = sum_S w.
 *   draw       out = the smallest j in S with sum_{i in S, i <= j} w_i > u * W_S, the sum in INDEX order.
 *   -inf logits (masked tokens) weigh 0 and are never returned while a finite logit exists.  Rows with +inf, NaN or no finite logit are
 *   the caller's error; the call still ends and returns an index in [0, n).
 * Arithmetic: w from one fp32 exp2 per element, then every sum in 2^-40 fixed point - exact integer additions.  Results are bit-identical
 * run to run and eager against graph replay; against the exact rule they differ by less than 1e-4 of normalised cumulative probability.
 *
 * u: uniforms[row] if `uniforms` (device float [rows], values in [0, 1)) is given; else Philox4x32-10 with counter (key_lo, key_hi, 0, 0)
 * and key (seed_lo, seed_hi), first output word, u = (word >> 8) * 2^-24, where key = row_keys[row] (device int64 [rows]) or the row
 * index when row_keys is null.  Counter-based: a replayed graph draws new numbers exactly when the caller changes row_keys on the device.
 * u_out (device float [rows], may be null) receives the uniform every row used.
 *
 * QS_EINVAL before any device call: logits or out null, n < 8 or n > 2^22, row_stride < n or not a multiple of 8, rows < 0, logits not
 * 16-byte, out / row_keys not 8-byte, a float / int32 array not 4-byte aligned.  rows == 0: QS_OK, no launch.
 * ---------------------------------------------------------------------------------------------------------- */
int qs_sample_rows(const void* logits, int64_t* out, int rows, int n, int64_t row_stride, float temperature, int top_k, float top_p,
                   const float* row_temperature, const int32_t* row_top_k, const float* row_top_p, const float* uniforms, uint64_t seed,
                   const int64_t* row_keys, float* u_out, qs_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Repetition, presence and frequency penalties (the three knobs of the reference's SamplingParams; no kernel counterpart there).  Edits
 * fp16 logit rows IN PLACE from the tokens in front of each row's position, on the device, in front of qs_argmax_rows / qs_sample_rows:
 * capturable, nothing allocated, nothing read back, no scratch.  The result is an fp16 row again.
 *
 * logits fp16 [batch * n_nodes, n] with row stride row_stride (elements).  history int32 [batch, cap] with row stride hist_stride >= cap;
 * lengths int32 [batch]; prompt_lens int32 [batch] or null (= 0); node_tokens int64 [batch, n_nodes] or null; parents int32 [n_nodes]
 * (ONE tree shape, as for the drafter; parents[0] = -1 by convention; may be null when node_tokens is).
 *
 * Row r = b * n_nodes + i.  Its CONTEXT is h[b, 0 .. L) with L = min(max(lengths[b], 0), cap), followed by node_tokens[b, j] for the nodes
 * j != 0 on the path root -> i, i itself included (the root is h[L-1] already).  node_tokens null: the history alone - with n_nodes = 1
 * the case of a plain decode step.  A sibling's token, or any node off the path, is in no context.  A node whose parent entry is not in
 * 0 .. j-1 hangs off the root (its path is the node alone; its children's paths go through it), as for qs_ngram_draft_tree.
 * For a token id t in [0, n):  c_all(t) = occurrences of t in the context;  c_gen(t) = occurrences at context positions >= prompt_lens[b]
 * (path tokens are all generated).  Ids outside [0, n), in the history or on the path, are ignored and no address is formed from them.
 *
 * The edit, for every t with c_all(t) > 0 and a logit other than -inf, from x = float(logit), every operation a float32 operation
 * rounded on its own (no fused multiply-add; IEEE division):
 *     x = x > 0 ? x / rep : x * rep                        (the HF / reference repetition rule)
 *     x = x - (freq * float(c_gen) + (c_gen > 0 ? pres : 0))
 *     logit = fp16(x), round to nearest even.
 * -inf stays -inf.  Ids not in the context, the padding between n and the row stride, and every row of a sequence whose parameters are
 * neutral (rep == 1, freq == 0, pres == 0) are NOT WRITTEN at all.  rep / freq / pres of sequence b: seq_repetition[b] / seq_frequency[b] /
 * seq_presence[b] where that device array (float [batch]) is given, else the scalar.  rep > 0 is the caller's duty.
 *
 * Counts are 16-bit: cap + 63 <= 65 535, anything larger is QS_EINVAL.  QS_EINVAL before any device call as well: logits, history or
 * lengths null, node_tokens without parents, n < 8 or n > 2^22, row_stride < n or not a multiple of 8, n_nodes outside 1 .. 64, cap < 1,
 * hist_stride < cap, batch < 0 or > 65 535 (one grid row per sequence), node_tokens not 8-byte or an int32 / float array not 4-byte aligned.  batch == 0: QS_OK, no launch.
 * One workgroup per (slice of 32 768 ids, sequence): the history is counted once per (sequence, slice), not once per row.  Bit-identical
 * run to run and eager against graph replay.
 * ---------------------------------------------------------------------------------------------------------- */
int qs_penalize_rows(void* logits, int64_t row_stride, int n, const int32_t* history, int64_t hist_stride, int cap,
                     const int32_t* lengths, const int32_t* prompt_lens, const int64_t* node_tokens, const int32_t* parents,
                     int batch, int n_nodes, float repetition, float frequency, float presence, const float* seq_repetition,
                     const float* seq_frequency, const float* seq_presence, qs_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * N-gram (prompt-lookup) tree drafter and the history it reads (no reference counterpart).  One draft tree per sequence, proposed from
 * the sequence's own tokens, on the device: capturable, nothing allocated, nothing read back.  With qs_history_append behind a
 * verification, history[b, :lengths[b]] is the text of sequence b and nothing of the loop draft -> verify -> accept -> commit -> record
 * crosses to the host.
 *
 * qs_ngram_draft_tree.  history int32 [batch, cap] with row stride hist_stride >= cap (elements); lengths int32 [batch]; per sequence
 * L = min(max(lengths[b], 0), cap) and h = history[b, :L]; h[L-1] is the root - the token whose K / V is not in the cache yet.  parents
 * int32 [n] (device; ONE tree shape per call, 1 <= n <= 64): node 0 is the root whatever parents[0] holds (-1 by convention), and
 * 0 <= parents[i] < i otherwise.  draft int64 [batch, n]:
 *   draft[b, 0] = h[L-1], or pad_token if L == 0.
 *   i >= 1, a = parents[i]:  c = h followed by the draft tokens on the path root -> a, the root's column excluded (len(c) = L + depth(a)).
 *     For a history position p, 1 <= p <= L-1, the match length is
 *         m(p) = max { m <= min(max_ngram, p) : h[p-1-j] == c[len(c)-1-j] for all 0 <= j < m }
 *     - matches are looked for in the history only, continuations are taken from the history only.  p is a candidate if
 *     m(p) >= min_match and h[p] differs from draft[b, s] of every earlier sibling (1 <= s < i, parents[s] == a).  draft[b, i] = h[p*] where
 *     p* maximises (m(p), p) lexicographically: the longest match, then the most recent.  No candidate: draft[b, i] = pad_token.
 *   A node whose parents[i] is not in 0 .. i-1 gets pad_token; its path is the node alone (its children see c = h followed by pad_token).
 *   A pad node's descendants follow the rule, pad_token being a token like any other in c.  Tokens compare as 64-bit integers (a history
 *   token is sign-extended).
 * 1 <= min_match <= max_ngram <= 16.  One workgroup per sequence; while L <= qs_ngram_draft_lds_tokens() the history is staged in LDS,
 * beyond it it is read from global memory - the results are the same.
 *
 * qs_history_append, after a verification.  past_lens int32 [batch] = lengths - 1 from BEFORE the lengths advanced; node_tokens int64
 * [batch, n] (the draft); accept_idx int32 [batch, max_accept], accept_lens int32 [batch] (m, cut to max_accept), next_token int64 [batch]:
 *   history[b, past + j] = node_tokens[b, accept_idx[b, j]]  for 1 <= j < m,      history[b, past + m] = next_token[b].
 * A write at an index outside 0 .. cap-1 is skipped, and so is one whose accept_idx entry names no node of the tree; m < 1 writes
 * nothing.  Nothing else in the row changes.  (Tokens are stored as int32.)
 *
 * QS_EINVAL before any device call: a null pointer, n or max_accept outside 1 .. 64, max_ngram / min_match outside the range above,
 * cap < 1, hist_stride < cap, batch < 0.  batch == 0: QS_OK, no launch.
 * ---------------------------------------------------------------------------------------------------------- */
int qs_ngram_draft_tree(const int32_t* history, int64_t hist_stride, int cap, const int32_t* lengths, const int32_t* parents,
                        int batch, int n, int max_ngram, int min_match, int64_t pad_token, int64_t* draft, qs_stream_t stream);
int qs_history_append(int32_t* history, int64_t hist_stride, int cap, const int32_t* past_lens, const int64_t* node_tokens,
                      const int32_t* accept_idx, const int32_t* accept_lens, const int64_t* next_token,
                      int batch, int n, int max_accept, qs_stream_t stream);
int qs_ngram_draft_lds_tokens(void);   /* history tokens the drafter stages in LDS (a compile-time constant of the library) */

/* ------------------------------------------------------------------------------------------------------------
 * Stop conditions (no reference counterpart: its stop checks are host Python).  qs_stop_update clips what one round - a decode step or a
 * tree verification - is about to emit at the first stop: a stop sequence completed in the generated text, or a length limit reached.
 * It runs between the walk and the commit, over the walk's own outputs, so that the launches behind it (qs_kv_cache_commit_path_layers,
 * the advance of the lengths, qs_history_append) commit, count and record the clipped path without knowing of it.  Capturable, nothing
 * allocated, everything integer: bit-identical run to run and eager against graph replay.
 *
 * Per sequence b.  L = min(max(lengths[b], 0), cap): the text length from BEFORE the round advances it; the text is history[b, 0 .. L)
 * (int32 [batch, cap], row stride hist_stride >= cap) followed by the emitted tokens e_1 .. e_m:
 *     m   = accept_lens[b] cut to 0 .. min(max_accept, 64); accept_lens null: m = 1; node_tokens or accept_idx null: m is cut to 0 .. 1;
 *     e_j = node_tokens[b, clamp(accept_idx[b, j], 0, n-1)]  for 1 <= j < m      (node_tokens int64 [batch, n], accept_idx int32 [batch, max_accept]);
 *     e_m = next_token[b]                                                          (int64 [batch]);
 * text position L - 1 + j holds e_j, the convention of qs_history_append; index j = 0 stands for the current token at position L - 1.
 * The token at text position p is history[b, p] for p < L and e_(p-L+1) otherwise; a position p < max(prompt_lens[b], 0) (int32 [batch]
 * or null = 0) or p >= cap holds NO token: it matches nothing.  Tokens compare as 64-bit integers.
 *
 * Stop table: stop_seqs int32 [num_stops, stop_width], stop_lens int32 [num_stops], 0 <= num_stops <= 32, 1 <= stop_width <= 8.  Row s is
 * stop_seqs[s, 0 .. stop_lens[s]); a row whose length is outside 1 .. stop_width, or that has a negative id in its used part, is off.
 * limit_lens int32 [batch] or null (no limit): the largest text length, prompt included.  finished int32 [batch], in and out: 0 = live,
 * 1 = stopped by a stop sequence, 2 = stopped by the length limit.
 *
 *     hit(j), 0 <= j <= m:  (a) limit_lens given and L + j >= limit_lens[b],  or
 *                           (b) j >= (check_root ? 0 : 1) and some row s that is on has, with l = stop_lens[s],
 *                               token(L - 1 + j - (l-1) + t) == stop_seqs[s, t] for all 0 <= t < l.
 *     k = the smallest j with hit(j); no hit: k = m and finished[b] stays 0.  On a hit finished[b] = 1 if (b) holds at k, else 2.
 *     finished[b] != 0 on entry: k = 0 and finished[b] is not written.
 *
 * Outputs.  accept_lens[b] = k in place (out_lens[b] = k where accept_lens is null).  next_token[b]: k == m - not written; 1 <= k < m -
 * e_k; k == 0 < m - history[b, L-1], the frozen token (not written if L == 0).  last_row[b] (int64 [batch] or null) =
 * b * n + clamp(accept_idx[b, k-1], 0, n-1) for 1 <= k < m, else not written.  Nothing else is written.  check_root = 1 is for the one
 * launch (with m = 0) that looks at the token a prefill drew.
 *
 * QS_EINVAL before any device call: history, lengths, next_token or finished null; accept_lens and out_lens both null; n or max_accept
 * outside 1 .. 64; num_stops outside 0 .. 32 or stop_width outside 1 .. 8; num_stops > 0 without stop_seqs / stop_lens; node_tokens null
 * with n > 1; accept_idx null with max_accept > 1; cap < 1; hist_stride < cap; check_root not 0 / 1; batch < 0; an int32 array not 4-byte
 * or an int64 array not 8-byte aligned.  batch == 0: QS_OK, no launch.  One wave64 per sequence.
 * ---------------------------------------------------------------------------------------------------------- */
int qs_stop_update(const int32_t* history, int64_t hist_stride, int cap, const int32_t* lengths, const int32_t* prompt_lens,
                   const int64_t* node_tokens, const int32_t* accept_idx, int32_t* accept_lens, int32_t* out_lens,
                   int64_t* next_token, int64_t* last_row, const int32_t* stop_seqs, const int32_t* stop_lens,
                   const int32_t* limit_lens, int32_t* finished, int batch, int n, int max_accept, int num_stops, int stop_width,
                   int check_root, qs_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Log-probabilities (no reference counterpart: its sampler layer computes them with torch ops on the host's schedule).  For every token
 * one round - a decode step or a tree verification - emits: its log-probability, its rank and a short top list, from the round's fp16
 * logit rows, on the device: capturable, nothing allocated, no workspace, nothing read back.  One entry covers a plain batch of rows
 * (n = max_accept = 1, node_tokens = accept_idx = accept_lens = null: row b is scored for next_token[b]) and an accepted path.
 *
 * logits fp16 [batch * n, n_vocab] with row stride row_stride (elements).  node_tokens int64 [batch, n] or null; accept_idx int32
 * [batch, max_accept] or null; accept_lens int32 [batch] or null; next_token int64 [batch]; lengths int32 [batch] or null.
 *
 * Slot (b, j), 1 <= j <= max_accept - the e_j of qs_stop_update, the row convention of qs_history_append, so after a clipping
 * qs_stop_update the same arrays describe the clipped path:
 *     m      = accept_lens[b] cut to 0 .. max_accept; accept_lens null: m = 1; node_tokens or accept_idx null: m is cut to 0 .. 1;
 *     live   iff j <= m; a dead slot writes nothing;
 *     row    = b * n + clamp(accept_idx[b, j-1], 0, n-1)        (accept_idx null: node 0) - the row whose head emitted the token;
 *     id t   = node_tokens[b, clamp(accept_idx[b, j], 0, n-1)]  for j < m,      next_token[b]  for j == m;
 *     column = L - 1 + j with L = max(lengths[b], 0) from BEFORE the round advances it - the token's text position -, or j - 1 where
 *              lengths is null.  A column >= out_cols is skipped.
 * Element (b, column) of out_lp (float) and out_rank (int32, may be null) lives at b * out_stride + column; the top lists out_top_ids
 * (int32) / out_top_lp (float) at (b * out_stride + column) * top, `top` entries each, 0 <= top <= 32.
 *
 * Per live slot, with the row x[0 .. n_vocab), T = seq_temperature[b] (float [batch]) where given, else `temperature`; T < 1e-5 (or NaN)
 * is taken as T = 1, so a greedy row reports the untempered distribution.  Top-k and top-p do not enter: the values describe
 * softmax(x / T) of the logits as handed in (the penalised logits when the caller penalised first).
 *     m = max x;  a_i = (x_i - m) * float(log2(e) / T) in fp32;  F_i = floor(exp2(a_i) * 2^40);  W = sum F_i, an exact 64-bit integer sum;
 *     lp(i) = (a_i - (log2(float(W)) - 40)) * ln 2 in fp32                   (exp2 / log2: the hardware's, ~1 ulp each)
 *     out_lp   = lp(t); t outside [0, n_vocab): NaN, and no address is formed from t; x_t = -inf: -inf.
 *     out_rank = 1 + #{i : key(x_i) > key(x_t)} + #{i < t : key(x_i) == key(x_t)}, key = the order-preserving 16-bit key of the fp16 value
 *                (-0 is +0); 0 when t is out of range.  An exact integer.
 *     top list = the first `top` ids in the order (key descending, index ascending) with their lp; only ids whose logit is not -inf are
 *                listed; if fewer than `top` exist, the tail is id -1 with lp -inf.  Ids are exact: no floating-point comparison decides
 *                them, a tie class of any size is cut by index.
 * Elements between n_vocab and the row stride are never read into a result.  Rows with NaN, +inf or no finite logit are the caller's
 * error; the call still ends.  All sums are integer sums: bit-identical run to run and eager against graph replay; against the exact
 * log-softmax |lp - exact| <= 1e-5 + 2^-21 * |lp|.
 *
 * QS_EINVAL before any device call: logits, next_token or out_lp null; n_vocab < 8 or > 2^22, row_stride < n_vocab or not a multiple of
 * 8; n or max_accept outside 1 .. 64; top outside 0 .. 32; top > 0 without out_top_ids and out_top_lp; node_tokens null with n > 1;
 * accept_idx null with max_accept > 1; out_cols < 0 or out_stride < out_cols; batch < 0 or > 65 535 (one grid row per sequence); logits
 * not 16-byte, an int64 array not 8-byte, an int32 / float array not 4-byte aligned.  batch == 0: QS_OK, no launch.  One workgroup of
 * 1024 threads per slot.
 * ---------------------------------------------------------------------------------------------------------- */
int qs_logprob_rows(const void* logits, int64_t row_stride, int n_vocab, const int64_t* node_tokens, const int32_t* accept_idx,
                    const int32_t* accept_lens, const int64_t* next_token, const int32_t* lengths, int batch, int n, int max_accept,
                    float temperature, const float* seq_temperature, int top, float* out_lp, int32_t* out_rank, int32_t* out_top_ids,
                    float* out_top_lp, int64_t out_stride, int out_cols, qs_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Constrained decoding (no reference counterpart): a TOKEN AUTOMATON restricts what every sequence may emit - a regular expression, a
 * choice list, a JSON shape of bounded depth, compiled on the host into two device tables - and the three entries below apply it inside
 * the decode round, on the device: capturable, nothing allocated, nothing read back, no scratch.  Integer rules only: bit-identical run
 * to run and eager against graph replay.
 *
 * Tables, shared by all sequences of a call (several grammars live in one table as disjoint state ranges):
 *     token_class int16 [n_vocab]   the class of every token id, in 0 .. C-1; a negative class, or one >= C: never allowed in any state.
 *     next        int32 [S, C], row stride next_stride >= C (elements).  next[s, c] >= 0: the state after a token of class c in state s;
 *                 a negative entry: not allowed in s.  A token t is allowed in s iff next[s, token_class[t]] >= 0.
 * A STATE outside 0 .. S-1, negative or not, is UNCONSTRAINED: -1 by convention, and QS_FSM_DEAD (-2), what a transition over a token
 * that is not allowed yields.
 *     T(st, t) = st                                  if st is outside 0 .. S-1   (unconstrained stays unconstrained, dead stays dead)
 *              = QS_FSM_DEAD                         if t is outside [0, n_vocab), or c = token_class[t] is outside [0, C), or next[st, c] < 0
 *              = next[st, c]                         otherwise.
 * No address is ever formed from an out-of-range token, class or state.
 *
 * qs_constrain_node_states: the state of every node of a draft tree - the state reached along the path root -> node.  state int32
 * [batch]; node_tokens int64 [batch, n] (column 0, the root's, is not read); parents int32 [n] (ONE tree shape, as for the drafter;
 * both may be null when n == 1); node_state int32 [batch, n], written:
 *     node_state[b, 0] = state[b];      node_state[b, i] = T(node_state[b, a], node_tokens[b, i])  for i >= 1, a = parents[i].
 * A parent entry not in 0 .. i-1 hangs the node off the root (a = 0), the convention of qs_ngram_draft_tree / qs_penalize_rows; its
 * children follow the rule through it.  A dead node only says "this node cannot be accepted": its parent's row, masked, never yields
 * its token.  One wave64 per sequence.
 *
 * qs_constrain_rows: the mask.  logits fp16 [rows, n_vocab] with row stride row_stride (elements), edited IN PLACE; row_state int32
 * [rows] - node_state flattened for a verification, state itself for a plain step.  For every row r with s = row_state[r] in 0 .. S-1:
 *     logits[r, t] = -inf (bits 0xFC00) for every t in [0, n_vocab) whose class is outside [0, C) or has next[s, class] < 0;
 * every other element keeps its bits, and so does the padding between n_vocab and the row stride.  A row whose state is outside
 * 0 .. S-1 is NOT WRITTEN at all (nor read).  One workgroup of 512 threads per (row, slice of the vocabulary); the allowed set of the
 * row's state is staged in LDS as one bit per class.
 *
 * qs_constrain_advance: the state after the round, behind the walk (and behind qs_stop_update where present), on the arrays of
 * qs_history_append.  node_state int32 [batch, n] or null; accept_idx int32 [batch, max_accept] or null; accept_lens int32 [batch] or
 * null; next_token int64 [batch]; state int32 [batch], in and out:
 *     k  = accept_lens[b] cut to 0 .. max_accept; accept_lens null: k = 1.    k == 0 (a frozen row, a path clipped to nothing): not written.
 *     st = node_state[b, clamp(accept_idx[b, k-1], 0, n-1)];  node_state or accept_idx null: st = state[b].
 *     st outside 0 .. S-1: state[b] is not written;  else state[b] = T(st, next_token[b]).
 * st is the state of the row that emitted e_k, and after a clipping qs_stop_update next_token[b] IS e_k.  One thread per sequence.
 *
 * QS_EINVAL before any device call: a null required pointer (state, token_class, next; node_state / logits, row_state / next_token);
 * n_vocab < 8 or > 2^22; row_stride < n_vocab or not a multiple of 8; C outside 1 .. 32 768; S < 1; next_stride < C; n or max_accept
 * outside 1 .. 64; node_tokens or parents null with n > 1; accept_idx null with max_accept > 1; batch / rows < 0 or > 2^24; logits or
 * token_class not 16-byte, an int64 array not 8-byte, an int32 array not 4-byte aligned.  batch == 0 / rows == 0: QS_OK, no launch.
 * ---------------------------------------------------------------------------------------------------------- */
#define QS_FSM_DEAD (-2)
int qs_constrain_node_states(const int32_t* state, const int64_t* node_tokens, const int32_t* parents, const int16_t* token_class,
                             int n_vocab, const int32_t* next, int64_t next_stride, int S, int C, int batch, int n,
                             int32_t* node_state, qs_stream_t stream);
int qs_constrain_rows(void* logits, int64_t row_stride, int n_vocab, const int32_t* row_state, const int16_t* token_class,
                      const int32_t* next, int64_t next_stride, int S, int C, int rows, qs_stream_t stream);
int qs_constrain_advance(int32_t* state, const int32_t* node_state, const int32_t* accept_idx, const int32_t* accept_lens,
                         const int64_t* next_token, const int16_t* token_class, int n_vocab, const int32_t* next, int64_t next_stride,
                         int S, int C, int batch, int n, int max_accept, qs_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * LoRA adapters next to the W4A8 linears (no reference counterpart): every SEQUENCE of a batch runs under its own low-rank adapter, or
 * under none.  A delta cannot be merged into 4-bit packed weights, so it is applied behind the base GEMM, per row, on the quantised
 * activations that GEMM read.  Rows are sequence-major with rows_per_seq rows per sequence (1 for a decode step, the chunk, the prompt
 * length, a tree's node count).  qs_lora_rows updates the fp16 output of the base linear IN PLACE: for row t of T, s = t / rows_per_seq,
 * a = seq_adapter[s] (int32, on the device).  a outside 0 .. slots-1 (-1 by convention: the base model): nothing of the row is read
 * or written, and no address is formed from a.  Otherwise, for every column n, g the segment n lies in:
 *     t_j       = float(x_scale[t]) * sum_k float(A[a, g r + j, k]) * x[t, k]            j = 0 .. r-1, float32, kept in float32
 *     out[t, n] = fp16(float(out[t, n]) + scaling[a] * sum_j float(B[a, n, j]) * t_j)
 * x int8 [T, K], row stride x_stride; x_scale fp16 [T]; A fp16 [slots, nseg r, K]; B fp16 [slots, N, r]; scaling float32 [slots];
 * out fp16 [T, N], row stride out_stride (elements).  The N columns are cut into nseg (1 .. 3) SEGMENTS by their ascending ends
 * seg_end0 .. seg_end{nseg-1} (the last one is N; the others are ignored) - q / k / v of a fused qkv, gate / up - and every segment has
 * its own r rows of A: a fused projection reads r columns of B per output, not nseg r columns of a block-diagonal matrix.
 * The float32 sums are taken in a fixed order (products of fp16 and int8 values are exact in float32): results are bit-identical run
 * to run and eager against graph replay; against another order of the sums, |got - y| <= 2^-11 |y| + 2^-24 + 2 (K + r + 4) 2^-24 M with
 * M = scaling sum_j |B| x_scale sum_k |A x|.  Two launches on `stream` (capturable): the float32 partial sums of the K slices travel
 * through `workspace` (workspace_size bytes, at least qs_lora_rows_workspace(T, K, r, nseg); not shared with a launch that may overlap).
 * No atomics, no in-launch waits.
 *
 * QS_EINVAL before any device call: a null pointer; r not 8, 16, 32 or 64; K not a multiple of 128 in 128 .. 2^20; N not a multiple of
 * 64 in 64 .. 2^22; nseg outside 1 .. 3; segment ends not ascending multiples of 64 or the last one not N; slots < 1; T < 0 or > 2^24;
 * rows_per_seq < 1 or not a divisor of T; x_stride < K or not a multiple of 16; out_stride < N or not a multiple of 8; out, x, A, B or
 * the workspace not 16-byte, scaling or seq_adapter not 4-byte, x_scale not 2-byte aligned; a workspace that is too small.  T == 0:
 * QS_OK, no launch.  qs_lora_rows_workspace: the bytes, or QS_EINVAL for a T, K, r or nseg outside those ranges.
 * ---------------------------------------------------------------------------------------------------------- */
int64_t qs_lora_rows_workspace(int T, int K, int r, int nseg);
int qs_lora_rows(void* out, int64_t out_stride, const int8_t* x, int64_t x_stride, const void* x_scale, const void* A, const void* B,
                 const float* scaling, const int32_t* seq_adapter, int slots, int T, int K, int N, int r, int rows_per_seq, int nseg,
                 int seg_end0, int seg_end1, int seg_end2, void* workspace, int64_t workspace_size, qs_stream_t stream);

/* ----------------------------------------------------------------------------------------------------------
 * Mixture-of-experts layers over the W4A8 linears (no reference counterpart: the reference's Mixtral block raises before routing -
 * its MoE kernels and `moe_helpers` were never released).  Pipeline of one sparse MLP on T token rows, E experts, k experts per token,
 * P = T k (token, expert) pairs:  qs_moe_route -> grouped gate_up GEMM (row_src = pair_token) -> qs_silu_and_mul_quant over the P
 * sorted rows -> grouped down GEMM -> qs_moe_combine.  Nothing is read back: every routing value stays on the device, every grid is
 * sized from (T, E, k, N, K), so the pipeline can be captured in a hipGraph.  Python: qserve_amd.moe; numpy restatement:
 * tests/_moe_cases.py.
 *
 * qs_moe_route (csrc/moe_route.hip): logits fp16 [T, E], row stride `logits_stride` elements, finite.  Per token the k largest
 * logits ordered by (value descending, expert index ascending), compared as the fp16 values they are: ties of any size go to the
 * lower index.  weights: softmax over all experts renormalised over the chosen k (the Mixtral rule) = softmax over the k chosen
 * logits l_0 >= l_1 >= ..., float32 op by op:  e_j = expf(float(l_j) - float(l_0));  s = ((e_0 + e_1) + ...) + e_{k-1};
 * w_j = e_j / s (IEEE division).  Outputs: expert_ids int32 [T, k]; weights float32 [T, k]; expert_offsets int32 [E + 1], the
 * exclusive prefix of the experts' pair counts (expert_offsets[E] = P); pair_token int32 [P], the source token of every position of
 * the expert-sorted order; pair_pos int32 [T, k], the sorted position of pair (t, j).  The sort is stable: inside an expert the pairs
 * are ordered by (t, j).  No atomic decides an output: results are bit-identical from run to run and under graph replay.  One launch
 * for T <= 256 and P <= 2048, four otherwise (select, per-chunk counts, scan, scatter) with the counts in `workspace`;
 * qs_moe_route_workspace gives the bytes a call needs (>= 16).  T == 0 writes the (all zero) offsets.
 * QS_EINVAL before any device call: null pointer; T outside 0 .. 2^24; E outside 1 .. 64; k outside 1 .. min(E, 8); P > 2^24;
 * logits_stride < E; logits not 2-byte or another tensor not 4-byte aligned; a workspace that is too small.
 *
 * qs_w4a8_per_chn_moe_gemm / qs_w4a8_per_group_moe_gemm (csrc/gemm_w4a8_moe.hip): for every sorted position p < P, with e the expert
 * whose range expert_offsets[e] <= p < expert_offsets[e + 1] holds p:  out[p, :] = W[e] x[row_src[p], :]  (row_src == NULL: x row p).
 * Weights: the reference's packed layout stacked over experts - qweight int8 [E, N, K/2], wscales (s1_scales) / w_szs (s1_szeros)
 * fp16 [E, N], per-group zeros (s2_zeros) / scales_i8 (s2_scales) int8 [E, K/128, N].  x int8 [x_rows, K] with row stride x_stride;
 * ascales / a_ssums fp16 [x_rows], indexed by the SOURCE row; out fp16 [P, N] with row stride out_stride.  Arithmetic of the dense
 * entries: exact int32 accumulation, the per-channel epilogue of the convention qs_set_gemm_epilogue selects at launch time, the
 * per-group epilogue of qs_w4a8_per_group_gemm - out[p] equals, bit for bit, the dense entry on expert e's tensors and that row.
 * A workgroup owns (expert, 64 channels, 16 mt sorted rows) and finds its expert from expert_offsets itself; the grid is the bound
 * ceil(P / (16 mt)) + E - 1 of qs_moe_gemm_plan, surplus workgroups leave at once, rows beyond an expert's range are not stored; rows
 * >= P of out and columns >= N of a padded row are never written.  Device inputs cannot move an access: offsets are clamped into
 * [0, P] (a range that runs backwards is empty), row_src values into [0, x_rows - 1].
 * QS_EINVAL before any device call: null pointer (row_src may be null); P outside 0 .. 2^21; E outside 1 .. 64; N not a multiple of
 * 64 or > 2^22; K not a multiple of 128 or > 2^20; x_stride < K or not a multiple of 16; out_stride < N or not a multiple of 8;
 * x_rows < 1, > 2^24, or < P without row_src; x, qweight or out not 16-byte, the weight scales not 8-byte, zeros / scales_i8 /
 * expert_offsets / row_src not 4-byte, the activation scales not 2-byte aligned.  P == 0: QS_OK, no launch.
 * qs_moe_gemm_plan: plan4 = {mt, waves per workgroup, row blocks launched, 64-channel units} - a pure function of (P, E, N, K)
 * (csrc/moe_plan.h); every plan computes the same bits.
 *
 * qs_moe_combine (csrc/moe_route.hip): out[t, :] = half(sum_j weights[t, j] * float(y[pair_pos[t, j], :])) for t < T: float32, j
 * ascending, the first product alone and each further one added to it, multiply and add rounded separately (no contraction), one
 * rounding to fp16.  y fp16 [T k, N] / out fp16 [T, N] with row strides; pair_pos values are clamped into [0, T k - 1].
 * QS_EINVAL before any device call: null pointer; T outside 0 .. 2^24; k outside 1 .. 8; N not a multiple of 64 in 64 .. 2^22; a
 * stride < N or not a multiple of 8; out or y not 16-byte, weights or pair_pos not 4-byte aligned.  T == 0: QS_OK, no launch.
 * ---------------------------------------------------------------------------------------------------------- */
int64_t qs_moe_route_workspace(int T, int E, int k);
int qs_moe_route(const void* logits, int64_t logits_stride, int T, int E, int k, int32_t* expert_ids, float* weights,
                 int32_t* expert_offsets, int32_t* pair_token, int32_t* pair_pos, void* workspace, int64_t workspace_size,
                 qs_stream_t stream);
int qs_moe_gemm_plan(int P, int E, int N, int K, int* plan4);
int qs_w4a8_per_chn_moe_gemm(const int8_t* x, int64_t x_stride, int x_rows, const int32_t* row_src, const int32_t* expert_offsets,
                             const int8_t* qweight, const void* wscales, const void* ascales, const void* w_szs, const void* a_ssums,
                             void* out, int64_t out_stride, int P, int E, int N, int K, qs_stream_t stream);
int qs_w4a8_per_group_moe_gemm(const int8_t* x, int64_t x_stride, int x_rows, const int32_t* row_src, const int32_t* expert_offsets,
                               const int8_t* qweight, const int8_t* zeros, const int8_t* scales_i8, const void* wscales,
                               const void* ascales, void* out, int64_t out_stride, int P, int E, int N, int K, qs_stream_t stream);
int qs_moe_combine(void* out, int64_t out_stride, const void* y, int64_t y_stride, const float* weights, const int32_t* pair_pos, int T,
                   int k, int N, qs_stream_t stream);

/* Timing tool (scripts/trace_attn.py): device-to-device copy of the first `bytes` of the split-KV workspace, where the
 * trace instantiation of the KV4 decode attention (qs_set_attention_variant(232)) leaves its s_memtime stamps.
 * (A library built with -DQS_RING_TRACE additionally exports qs_debug_ring_trace(void* buf) for scripts/trace_gemm.py;
 * it is not part of the shipped ABI.) */
int qs_debug_copy_split_workspace(void* dst, size_t bytes);

/* Tests: where the RoPE cos / sin values of the current device come from.  The writers and the decode kernels read a library-managed
 * table where one covers a row's position and evaluate the same values in the kernel elsewhere; the tables live in 8 slots per device,
 * keyed by (base, length), and are never freed.  *slots_used = occupied slots, *longest_len_for_base = rows of the longest table whose
 * base equals `base` exactly (0: none - every position of that base is evaluated in the kernel).  Host only, read only: no launch,
 * no allocation, nothing but hipGetDevice; safe inside a stream capture.  QS_EINVAL: null output, no current device. */
int qs_debug_rope_table_state(float base, int* slots_used, int* longest_len_for_base);

/* ----------------------------------------------------------------------------------------------------------
 * RoPE frequency profiles (no reference counterpart: the reference reads `rope_scaling` and never forwards it to its kernels).
 * A profile stands in for a rotary base wherever one is passed: 64 float32 denominators denom[pair] and one float32 mscale, with
 *     ang = (float)pos / denom[pair];   c = (float)cos((double)ang) * mscale;   s = (float)sin((double)ang) * mscale
 * (float32 division as for a base, ONE float32 multiply; mscale == 1.0f is exact) - the single definition behind the profile's tables
 * and every in-kernel evaluation; the rotation itself is the one of a base.  llama3, linear and YaRN scaling are such profiles
 * (Python: qserve_amd.rope computes them from a config's rope_scaling).
 *
 * qs_rope_profile_register: *key_out = -(id + 1), a NEGATIVE float, to be passed as `rotary_base` / `rotary_embedding_base` of
 * qs_apply_bias_rope_update_kv_cache, qs_append_rope_update_kv_cache, qs_append_tree_rope_update_kv_cache, qs_single_query_attention
 * and qs_single_query_attention_quant - eagerly or inside a stream capture.  Ids are process-wide and content-addressed: the same 64
 * denominators and mscale, bitwise, give the same key on every device; at most 8 profiles per process.  Registration is eager: it
 * builds the profile's cos / sin table of `table_positions` rows (1 .. 32768) on the current device, on the NULL stream, and waits for
 * it before publishing it; register once per device that uses the key.  Profile tables live beside the 8 slots of plain bases, not in
 * them (qs_debug_rope_table_state does not see them), and are never freed or moved: captured graphs hold their addresses.  An eager
 * call that needs more rows builds a longer table for the key (the old one stays alive); rows that no table covers - inside a capture,
 * beyond the 32 768 rows of the writers' tables - are evaluated in the kernel from the profile's 64 denominators in device memory,
 * with the same values.  Plain (positive) bases keep their code path and their bytes.
 *
 * QS_EINVAL with a message, nothing launched: null pointer; pairs != 64; table_positions outside 1 .. 32768; a denominator or mscale
 * that is not positive and finite; a ninth distinct profile; a call inside a stream capture (or a table that cannot be allocated).
 * Every entry that rotates returns QS_EINVAL for a negative base that is no registered key, and for a key on a device where it was
 * not registered.
 *
 * qs_debug_rope_profile_state (tests): *profiles_used = profiles of the process, *longest_table_len = rows of the longest table of
 * `key` on the current device (0: not a key, or not registered there).  Host only, read only; safe inside a stream capture.
 * ---------------------------------------------------------------------------------------------------------- */
int qs_rope_profile_register(const float* denom, int pairs /* must be 64 */, float mscale, int table_positions, float* key_out);
int qs_debug_rope_profile_state(float key, int* profiles_used, int* longest_table_len);

/* ----------------------------------------------------------------------------------------------------------
 * Page pool (no reference counterpart: its block manager is host Python).  A pool has N pages per layer, one index space for the K and
 * the V pool of every layer; each pool tensor holds N + 1 pages of page_bytes bytes, and page N is the SINK: never on the free list,
 * named by every table entry that names no owned page, so that no entry is ever null or stale.  The two entries move pages between the
 * free stack and the rows of the per-layer pointer tables on the device: capturable, nothing allocated, nothing read back, all integer.
 *
 * State, filled in place.  free_list int32 [N]: a stack, free_list[0 .. count) are the free indices, popped from the top; count int32
 * [1]; page_ids int32 [batch, max_blocks]: the physical page of logical page j of row b, or -1; owned int32 [batch]: pages a row owns
 * (its logical pages 0 .. owned - 1); starved int32 [batch]: set when a row was refused pages; error int32 [1]: set on a broken
 * invariant.  layer_tables int64 [num_layers]: the addresses of the layers' pointer tables int64 [batch, 2, max_blocks] (what
 * qs_kv_cache_commit_path_layers takes); layer_bases int64 [num_layers, 2]: the K / V pool base addresses.  The table entry of page id
 * in layer l is layer_bases[l, kv] + id * page_bytes; the sink's is layer_bases[l, kv] + N * page_bytes.
 *
 * qs_pages_reserve.  lengths int32 [batch]; extra_rows int32 [batch] or null; finished int32 [batch] or null, in and out.  Per row b:
 *     e_b    = max(extra_rows[b], 0) if extra_rows is given, otherwise extra;
 *     need_b = min(ceil((max(lengths[b], 1) - 1 + e_b) / 64), max_blocks)    - the slots a round of e_b new tokens writes;
 *     grow_b = 0 if finished is given and finished[b] != 0, otherwise max(need_b - owned[b], 0);
 *     S_b    = grow_0 + .. + grow_b, the inclusive prefix in row order;
 *     row b is SERVED iff S_b <= count.
 * A served row's j-th new page, 0 <= j < grow_b, is id = free_list[count - 1 - (S_b - grow_b + j)]: page_ids[b, owned[b] + j] = id, and
 * entry (b, kv, owned[b] + j) of the K and V tables of all layers becomes that page's address; then owned[b] += grow_b.  A row with
 * grow_b > 0 that is not served gets nothing: starved[b] = 1, and finished[b] = 3 (no pages) where finished is given and finished[b]
 * == 0.  count drops by the largest served S_b.  Rows are served all or nothing and the rule is deterministic; with grow <= 1 per row -
 * every plain step - it is exactly first come in row order.  With larger grows a row may be refused although a lone page remains, and
 * a later row whose smaller demand would still fit is refused with it (the prefix does not skip).
 *
 * qs_pages_release.  rows_mask int32 [batch]: rows with a non-zero entry are MASKED.  With E_b the exclusive prefix of owned over the
 * masked rows, in row order: free_list[count + E_b + j] = page_ids[b, j] for 0 <= j < owned[b] - rows push their pages back in row
 * order, then in logical page order -, page_ids[b, j] = -1, the table entries (b, kv, j) of all layers become the sink's address,
 * owned[b] = 0, starved[b] = 0; count rises by the masked rows' total.  Other rows keep everything.
 *
 * Broken invariants: count outside 0 .. N, an owned[b] outside 0 .. max_blocks, a page id outside 0 .. N - 1 among those about to be
 * popped (reserve) or pushed (release), or a release that would raise count above N: error[0] = 1 and the launch changes NOTHING else.
 * No address is formed from an unchecked or unclamped index.  What a table already holds is not checked.
 *
 * QS_EINVAL before any device call: a null pointer (extra_rows and finished may be null); num_pages < 1; max_blocks or num_layers < 1;
 * page_bytes < 1; num_pages * num_layers >= 2^30; batch outside 0 .. 1024; batch * max_blocks * 2 * num_layers >= 2^31; extra < 0; an
 * int32 array not 4-byte, layer_tables or layer_bases not 8-byte aligned.  batch == 0: QS_OK, no launch.  One launch of ONE workgroup
 * each: a wave64 shuffle scan, the waves' totals through LDS, rows beyond the workgroup's 256 threads by a strided loop; no atomics.
 * ---------------------------------------------------------------------------------------------------------- */
int qs_pages_reserve(int32_t* free_list, int32_t* count, int32_t* page_ids, int32_t* owned, int32_t* starved, int32_t* error,
                     const int64_t* layer_tables, const int64_t* layer_bases, const int32_t* lengths, const int32_t* extra_rows,
                     int32_t* finished, int batch, int max_blocks, int num_layers, int num_pages, int64_t page_bytes, int extra,
                     qs_stream_t stream);
int qs_pages_release(int32_t* free_list, int32_t* count, int32_t* page_ids, int32_t* owned, int32_t* starved, int32_t* error,
                     const int64_t* layer_tables, const int64_t* layer_bases, const int32_t* rows_mask, int batch, int max_blocks,
                     int num_layers, int num_pages, int64_t page_bytes, qs_stream_t stream);

/* ----------------------------------------------------------------------------------------------------------
 * Reference counts over the page pool: a page may have more than one HOLDER, so that rows can share the whole pages of a common
 * prefix (qserve_amd/prefix.py).  A holder is a (row, column) of page_ids that names the page, or the prefix cache (at most one hold
 * per page).  Two more state tensors, filled in place: refs int32 [N]: the holders of page id - 0 means free, i.e. on the free stack
 * -; scratch int32 [2 * N]: all zero between launches (every launch leaves it as it found it).  A pool either runs the four entries
 * below and never qs_pages_reserve / qs_pages_release, or the other way round.  One launch of ONE workgroup each, capturable.
 *
 * qs_pages_reserve_refs.  The rule of qs_pages_reserve, and refs[id] = 1 for every popped id; a popped id with refs[id] != 0 is a
 * broken invariant.  The same kernel (qs_pages_reserve runs it without refs).
 *
 * qs_pages_hold.  take int32 [batch]; src int32 [batch, max_blocks]; hold_ids int32 [num_hold] (null when num_hold == 0).  For every
 * row b with take[b] > 0: page_ids[b, j] = src[b, j] for 0 <= j < take[b], entry (b, kv, j) of the K and V tables of all layers
 * becomes that page's address, owned[b] = take[b].  refs[id] += the number of (b, j), j < take[b], with src[b, j] == id, + the number
 * of k with hold_ids[k] == id.  The same page may be mapped into several rows in one launch.  Broken invariants: take[b] outside
 * 0 .. max_blocks; take[b] > 0 where owned[b] != 0; a named id (src[b, j] with j < take[b], hold_ids[k]) outside 0 .. N - 1 or with
 * refs[id] == 0 (a free page cannot be shared); an id twice in hold_ids.
 *
 * qs_pages_unhold.  rows_mask int32 [batch] (non-zero: MASKED); drop_ids int32 [num_drop] (null when num_drop == 0).  H, the list of
 * holds given up, is page_ids[b, j] for the masked rows b in row order, 0 <= j < owned[b] in logical page order, followed by
 * drop_ids in order; g(id) is the number of positions of H that hold id.  refs[id] -= g(id); a page whose count reaches 0 is FREED.
 * With f_0 < f_1 < .. the positions of H that are the FIRST occurrence of a freed page: free_list[count + i] = H[f_i], and count
 * rises by their number.  The masked rows end as after qs_pages_release: page_ids[b, j] = -1, the table entries the sink's address,
 * owned[b] = starved[b] = 0.  Broken invariants: count outside 0 .. N; an owned[b] outside 0 .. max_blocks; an id of H outside
 * 0 .. N - 1; g(id) > refs[id]; count rising above N.
 *
 * qs_pages_fork.  src_rows int32 [batch]; lengths int32 [batch]; finished int32 [batch] or null, in and out.  Rows branch off running
 * texts: they share the whole pages of their source and get a copy of its partly filled tail page.  TWO launches on the stream, no
 * scratch.  Row d is a DESTINATION iff s = src_rows[d] >= 0 (any negative value: the row is not touched).  For a destination:
 *     len = max(lengths[s], 1);  w = (len - 1) / 64;  t = (len - 1) % 64;  need = w + (t > 0 ? 1 : 0)
 * - slot len - 1 is the first slot any writer of the text still writes, so pages 0 .. w - 1 are never written again and page w, if t
 * > 0, holds t slots that both texts read.  The source COVERS the fork iff need <= max_blocks and owned[s] >= need.  A destination
 * whose source does not cover it is REFUSED.  Every other destination asks for grow_d = (t > 0 ? 1 : 0) fresh pages; with S_d the
 * inclusive prefix of grow in row order (0 for rows that ask nothing), it is SERVED iff grow_d == 0 or S_d <= count, otherwise
 * REFUSED; the s-th popped id is free_list[count - 1 - s], and count drops by the largest served S_d.  A served destination:
 * page_ids[d, j] = page_ids[s, j] for 0 <= j < w, with refs += 1 per naming (d, j) (several destinations may name one page);
 * page_ids[d, w] = free_list[count - S_d] with refs = 1, if t > 0; entry (d, kv, j) of the K and V tables of all layers becomes the
 * page's address for 0 <= j < need; owned[d] = need.  A refused destination holds nothing: starved[d] = 1, and finished[d] = 3 where
 * finished is given and finished[d] == 0.  Broken invariants: count outside 0 .. N; an owned[b] outside 0 .. max_blocks; s >= batch;
 * s == d; src_rows[s] >= 0 (a source is no destination of the same launch); owned[d] != 0; page_ids[s, j] for j < min(need,
 * owned[s]) outside 0 .. N - 1 or with refs == 0; a popped id outside 0 .. N - 1 or with refs != 0.
 * The second launch, a grid over (row, layer x K / V), copies the page_bytes bytes of page page_ids[s, w] to page page_ids[d, w] in
 * every pool, for every destination that the first launch served with t > 0 - which it reads from the state: error[0] == 0,
 * starved[d] == 0 (so a destination still marked by an EARLIER refusal is mapped but not copied: release a row before it becomes
 * one), owned[d] == need <= owned[s], the two ids in range and different, the two table entries those pages' addresses.  The whole
 * page is copied: the allocator does not know a page's layout, and readers mask the slots beyond a text.  16-byte vectors where
 * page_bytes and both addresses are multiples of 16, bytes otherwise.
 *
 * A broken invariant: error[0] = 1 and the launch changes NOTHING else (the scratch is zero again).  The state after a launch is a
 * function of the state before it, the order of the free stack included: the only atomics are integer add and max on refs and the
 * scratch, whose result no arrival order changes.  Vector stores only; no address is formed from an unchecked or unclamped index.
 *
 * QS_EINVAL before any device call: what qs_pages_reserve / qs_pages_release refuse (take, src and rows_mask may not be null); refs
 * null; scratch null (hold, unhold); num_hold / num_drop outside 0 .. num_pages; a null id list with a positive number; an int32
 * array not 4-byte aligned.  batch == 0 (and, for hold and unhold, no ids): QS_OK, no launch.  qs_pages_fork: src_rows and lengths
 * may not be null, finished may.
 * ---------------------------------------------------------------------------------------------------------- */
int qs_pages_reserve_refs(int32_t* free_list, int32_t* count, int32_t* page_ids, int32_t* owned, int32_t* starved, int32_t* error,
                          const int64_t* layer_tables, const int64_t* layer_bases, int32_t* refs, const int32_t* lengths,
                          const int32_t* extra_rows, int32_t* finished, int batch, int max_blocks, int num_layers, int num_pages,
                          int64_t page_bytes, int extra, qs_stream_t stream);
int qs_pages_hold(int32_t* free_list, int32_t* count, int32_t* page_ids, int32_t* owned, int32_t* starved, int32_t* error,
                  const int64_t* layer_tables, const int64_t* layer_bases, int32_t* refs, int32_t* scratch, const int32_t* take,
                  const int32_t* src, const int32_t* hold_ids, int num_hold, int batch, int max_blocks, int num_layers, int num_pages,
                  int64_t page_bytes, qs_stream_t stream);
int qs_pages_unhold(int32_t* free_list, int32_t* count, int32_t* page_ids, int32_t* owned, int32_t* starved, int32_t* error,
                    const int64_t* layer_tables, const int64_t* layer_bases, int32_t* refs, int32_t* scratch, const int32_t* rows_mask,
                    const int32_t* drop_ids, int num_drop, int batch, int max_blocks, int num_layers, int num_pages, int64_t page_bytes,
                    qs_stream_t stream);
int qs_pages_fork(int32_t* free_list, int32_t* count, int32_t* page_ids, int32_t* owned, int32_t* starved, int32_t* error,
                  const int64_t* layer_tables, const int64_t* layer_bases, int32_t* refs, const int32_t* src_rows,
                  const int32_t* lengths, int32_t* finished, int batch, int max_blocks, int num_layers, int num_pages, int64_t page_bytes,
                  qs_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Beam search (no reference counterpart): the W best continuations of every group of W rows of a fixed batch, and the in-place move of
 * the rows whose text changes - on the device: capturable, nothing allocated, nothing read back, no scratch.
 *
 * qs_beam_select.  logits fp16 [batch, n_vocab] with row stride row_stride (elements), as the head left them (penalised, masked); cum
 * float [batch], the score of every row's text; finished int32 [batch]; tokens int64 [batch], every row's current token; width W,
 * 1 .. 32, batch % W == 0: rows g * W .. g * W + W - 1 form group g.  Outputs: parent int32 [batch] (absolute row indices), next_token
 * int64 [batch], cum_out float [batch] (must not alias cum), moved int32 [batch] or null (1 where parent[d] != d), src_rows int32 [batch]
 * or null (parent[d] where moved, else -1: what qs_pages_fork takes), and the candidate workspace cand_ids int32 [batch, W], cand_lp
 * float [batch, W], an output too.  TWO launches on the stream.
 *
 * A row b is DEAD iff cum[b] == -inf, FROZEN iff it is not dead and finished[b] != 0, LIVE otherwise.
 *
 * Launch 1, one workgroup of 1024 threads per row: a live row writes into cand_ids[b, :] / cand_lp[b, :] the top list qs_logprob_rows
 * defines for top = W at T = 1 - (key descending, index ascending), only logits other than -inf, the tail id -1 / lp -inf - with the
 * same operations in the same order: ids and lp are BIT-IDENTICAL to what qs_logprob_rows writes for that row.  A dead or frozen row
 * reads no logit and writes ids -1 / lp -inf.
 *
 * Launch 2, one wave per group, integer operations and single fp32 operations rounded on their own; no atomics.  The CANDIDATES of a
 * group: for a live row b every (b, r) with cand_ids[b, r] >= 0, score = cum[b] + cand_lp[b, r] (one fp32 add), token = cand_ids[b, r];
 * for a frozen row b the one candidate (b, 0) with score = cum[b], token = tokens[b].  A candidate whose score is -inf (or NaN) is
 * dropped.  Order: score descending as fp32 values (-0 equals +0), then row ascending, then r ascending.  The first min(W, count)
 * candidates are CHOSEN.  Slots: for every row p with a chosen candidate, p's first chosen candidate takes slot p; the remaining chosen
 * candidates, in order, take the slots of the rows without one, in ascending row order.  Slot d with a candidate (p, token, score):
 * parent[d] = p, next_token[d] = token, cum_out[d] = score; a slot left over: parent[d] = d, next_token[d] = tokens[d], cum_out[d] =
 * -inf.  So every source of a move is a row that stays: parent[parent[d]] == parent[d] - moved / src_rows meet what qs_pages_unhold
 * followed by qs_pages_fork ask of a mask and its sources, and where every row keeps one child nothing moves.
 * Rows with NaN, +inf or no finite logit are the caller's error; the call still ends.  The result is a function of the inputs alone:
 * bit-identical run to run and eager against graph replay.
 *
 * QS_EINVAL before any device call: logits, cum, finished, tokens, parent, next_token, cum_out, cand_ids or cand_lp null; width outside
 * 1 .. 32; batch < 0 or > 65 535 or not a multiple of width; n_vocab < 8 or > 2^22, row_stride < n_vocab or not a multiple of 8; cum_out
 * == cum; logits not 16-byte, an int64 array not 8-byte, an int32 / float array not 4-byte aligned.  batch == 0: QS_OK, no launch.
 *
 * qs_rows_move.  parent int32 [batch]; bases / row_bytes: HOST arrays of `num` (0 .. 16) device base addresses and row sizes in bytes
 * (1 .. 2^31) - tensor i is [batch] rows of row_bytes[i] bytes at bases[i]; they travel by value in the kernel argument; error int32
 * [1].  ONE launch, a grid over (tensor, row): for every tensor and every row d with p = parent[d] != d, the bytes of row d become the
 * bytes of row p - 16-byte vectors where the base and the row size are multiples of 16, bytes otherwise.  A p outside 0 .. batch - 1,
 * or with parent[p] != p (a source that is itself a destination), sets error[0] = 1 and row d is skipped in every tensor: no address
 * is formed from an unchecked index, and since every source stays the move needs no staging.  Vector stores only; no scratch.
 * QS_EINVAL before any device call: parent or error null or not 4-byte aligned; batch < 0 or > 65 535; num outside 0 .. 16; bases or
 * row_bytes null with num > 0; a null base; a row size outside 1 .. 2^31.  batch == 0 or num == 0: QS_OK, no launch.
 * ---------------------------------------------------------------------------------------------------------- */
int qs_beam_select(const void* logits, int64_t row_stride, int n_vocab, const float* cum, const int32_t* finished, const int64_t* tokens,
                   int batch, int width, int32_t* parent, int64_t* next_token, float* cum_out, int32_t* moved, int32_t* src_rows,
                   int32_t* cand_ids, float* cand_lp, qs_stream_t stream);
int qs_rows_move(const int32_t* parent, int batch, const void* const* bases, const int64_t* row_bytes, int num, int32_t* error,
                 qs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* QSERVE_AMD_H */
