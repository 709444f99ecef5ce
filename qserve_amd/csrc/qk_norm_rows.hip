// qk_norm_rows.hip -- per-head RMSNorm of the query and key heads (Qwen3's q_norm / k_norm), in place on the packed fp16 qkv rows, for
// MI355X (gfx950): the launch between the qkv GEMM (and its LoRA delta) and whatever rotates the rows next - the prefill, append and tree
// writers or a decode attention.  DESIGN.md 10 ("Q/K norm"); the rule is the header comment of qs_qk_norm_rows in include/qserve_amd.h.
// This file holds ONE kernel:
//
//   qk_norm_rows_kernel  a head is 128 halves = 256 bytes.  One DPP row of 16 lanes owns one head slot, 16 bytes per lane: one
//              global_load_dwordx4, one global_store_dwordx4.  A wave holds 4 slots, a workgroup of 4 waves 16 CONSECUTIVE slots.  Slot
//              s = token * (H + Hkv) + h sits at column h * 128 of its token's row: the q heads and the k heads are adjacent in the packed
//              row, so the address has no q / k case - h < H only picks which of the two weight vectors the lane keeps (both are loaded, 16
//              bytes each per lane, ahead of the row's own load; they are 512 bytes that never leave the caches).  The v heads and the
//              padding of a row are never addressed.
//                1. 8 squares per lane, summed in the lane's element order with one fma each;
//                2. four cross-lane steps inside the row on the DPP crossbar: quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror,
//                   row_mirror.  Each step adds two values that both lanes of the pair hold (a + b in one, b + a in the other), so all 16
//                   lanes end with the same bits and the order of the sum is fixed: bit-identical run to run and under graph replay;
//                3. r = 1 / sqrt(sum / 128 + eps), the correctly rounded float32 division and square root (hipcc's default);
//                4. t = fp16(x * r), y = fp16(w * t): two roundings to fp16, as transformers' Qwen3RMSNorm makes them on an fp16 input.
//              No LDS, no barrier, no workspace, no atomics.  A DPP source is always a lane of the same row, and a row is wholly inside
//              or wholly outside the launch (a slot is a row), so the rows of the last workgroup that have no slot just leave.
//              The stores are ordinary ones: the next launch reads these rows, they should stay in L2.
#include "common.h"

namespace {

constexpr int QKN_DH = 128;                              // head dimension: the only one the library has kernels for
constexpr int QKN_LANES = 16;                            // lanes per head slot: one DPP row, 8 halves each
constexpr int QKN_THREADS = 256;                         // 4 waves
constexpr int QKN_SLOTS = QKN_THREADS / QKN_LANES;       // 16 head slots per workgroup
constexpr long long QKN_MAX_SLOTS = 1ll << 27;           // grid * block stays below 2^32 threads
static_assert(QKN_LANES * 8 == QKN_DH, "16 lanes of 8 halves are one head");

// the sum of a 16-lane DPP row in every lane of it; a fixed order (see the header comment).  The whole row must be active.
__device__ __forceinline__ float row16_sum(float v) {
#pragma clang fp contract(off)
#define QS_DPP(ctrl) __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), ctrl, 0xF, 0xF, true))
    v = v + QS_DPP(0xB1);    // quad_perm [1,0,3,2]
    v = v + QS_DPP(0x4E);    // quad_perm [2,3,0,1]
    v = v + QS_DPP(0x141);   // row_half_mirror
    v = v + QS_DPP(0x140);   // row_mirror
#undef QS_DPP
    return v;
}

// grid = ceil(slots / 16), 256 threads.  The launcher checks the sizes, the stride and the alignment.
__global__ __launch_bounds__(QKN_THREADS) void qk_norm_rows_kernel(_Float16* __restrict__ qkv, const _Float16* __restrict__ q_weight,
                                                                   const _Float16* __restrict__ k_weight, u32 slots, u32 heads,
                                                                   u32 q_heads, long long stride0, float eps) {
    const u32 sub = threadIdx.x & (QKN_LANES - 1);
    const u32 slot = blockIdx.x * QKN_SLOTS + (threadIdx.x >> 4);
    if (slot >= slots) return;                            // (whole DPP rows leave: see the header comment)
    const h8 wq = *reinterpret_cast<const h8*>(q_weight + sub * 8);
    const h8 wk = *reinterpret_cast<const h8*>(k_weight + sub * 8);
    const u32 token = slot / heads, h = slot - token * heads;
    _Float16* p = qkv + (long long)token * stride0 + (long long)(h * QKN_DH + sub * 8);
    const h8 x = *reinterpret_cast<const h8*>(p);
    const h8 w = h < q_heads ? wq : wk;

    float xf[8], ss = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        xf[i] = (float)x[i];
        ss = __builtin_fmaf(xf[i], xf[i], ss);
    }
    ss = row16_sum(ss);
    const float r = 1.0f / __builtin_sqrtf(ss * (1.0f / QKN_DH) + eps);
    h8 y;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const _Float16 t = (_Float16)(xf[i] * r);
        y[i] = (_Float16)((float)w[i] * (float)t);
    }
    *reinterpret_cast<h8*>(p) = y;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int qs_qk_norm_rows(void* qkv, const void* q_weight, const void* k_weight, int num_tokens, int num_heads, int num_kv_heads,
                               int head_dim, int64_t qkv_stride0, float eps, qs_stream_t stream) {
    QS_REQUIRE(qkv && q_weight && k_weight, "qk_norm_rows: null pointer");
    QS_REQUIRE(eps > 0.f, "qk_norm_rows: eps=%g (must be > 0: an all-zero head has to stay finite)", (double)eps);
    QS_REQUIRE(num_tokens >= 0, "qk_norm_rows: num_tokens=%d", num_tokens);
    QS_REQUIRE(num_heads > 0 && num_kv_heads > 0 && num_heads % num_kv_heads == 0, "qk_norm_rows: bad head counts H=%d Hkv=%d", num_heads,
               num_kv_heads);
    if (head_dim != QKN_DH) {
        qs_set_error("qk_norm_rows: only head_dim=128 is supported");
        return QS_ENOSUP;
    }
    QS_REQUIRE(qkv_stride0 >= ((int64_t)num_heads + 2 * (int64_t)num_kv_heads) * QKN_DH && qkv_stride0 % 8 == 0,
               "qk_norm_rows: qkv_stride0=%lld must hold a row of (H + 2 Hkv) * 128 = %lld halves and keep 16-byte alignment",
               (long long)qkv_stride0, ((long long)num_heads + 2 * (long long)num_kv_heads) * QKN_DH);
    QS_REQUIRE(aligned16(qkv) && aligned16(q_weight) && aligned16(k_weight), "qk_norm_rows: qkv and the weights must be 16-byte aligned");
    const long long heads = (long long)num_heads + num_kv_heads, slots = (long long)num_tokens * heads;
    QS_REQUIRE(slots <= QKN_MAX_SLOTS, "qk_norm_rows: %d tokens of %lld heads are more than %lld head slots", num_tokens, heads, QKN_MAX_SLOTS);
    if (num_tokens == 0) return QS_OK;
    hipLaunchKernelGGL(qk_norm_rows_kernel, dim3((unsigned)((slots + QKN_SLOTS - 1) / QKN_SLOTS)), dim3(QKN_THREADS), 0, (hipStream_t)stream,
                       (_Float16*)qkv, (const _Float16*)q_weight, (const _Float16*)k_weight, (u32)slots, (u32)heads, (u32)num_heads,
                       (long long)qkv_stride0, eps);
    return qs_launch_status("qk_norm_rows");
}
