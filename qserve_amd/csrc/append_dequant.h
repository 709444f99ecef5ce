// append_dequant.h -- the leaves the append attention kernels (append_attention.hip, append_attention_split.hip, append_tree.hip)
// share: the exact KV4 / KV8 -> fp16 de-quantisation of 8 consecutive dims of a cached token (the decode kernels' values), the scalar
// form of a page address for the LDS-DMA's base operand, the launch geometry and the argument checks.  The page staging and the key
// loop built from these leaves are append_walk.h.
#pragma once
#include "flash_tile.h"

namespace qs_append {

using namespace qs_flash;

constexpr int MAX_G = 8;          // query heads per KV head (the decode kernels' range)

// exact uint4 -> fp16 for the 8 nibbles of x, in the order (e0,e4),(e1,e5),(e2,e6),(e3,e7) (the decode kernels' form, attention.hip)
__device__ __forceinline__ void nib8_to_h2(u32 x, h2 (&o)[4]) {
    const u32 t = x >> 8;
    const u32 w0 = (x & 0x000F000Fu) | 0x64006400u;
    const u32 w1 = (x & 0x00F000F0u) | 0x64006400u;
    const u32 w2 = (t & 0x000F000Fu) | 0x64006400u;
    const u32 w3 = (t & 0x00F000F0u) | 0x64006400u;
    const h2 k1024 = {(_Float16)1024.f, (_Float16)1024.f};
    const h2 k16 = {(_Float16)0.0625f, (_Float16)0.0625f};
    const h2 km64 = {(_Float16)-64.f, (_Float16)-64.f};
    o[0] = __builtin_bit_cast(h2, w0) - k1024;
    o[1] = __builtin_elementwise_fma(__builtin_bit_cast(h2, w1), k16, km64);
    o[2] = __builtin_bit_cast(h2, w2) - k1024;
    o[3] = __builtin_elementwise_fma(__builtin_bit_cast(h2, w3), k16, km64);
}

// A wave-uniform pointer as the scalar pair the LDS-DMA's base operand wants: a load behind an asm statement with a memory clobber
// is issued as a vector load, and its (uniform) result lives in vector registers.
__device__ __forceinline__ const uint8_t* scalar_ptr(int64_t p) {
    const u32 lo = __builtin_amdgcn_readfirstlane((u32)(uint64_t)p), hi = __builtin_amdgcn_readfirstlane((u32)((uint64_t)p >> 32));
    return reinterpret_cast<const uint8_t*>(((uint64_t)hi << 32) | lo);
}

// 8 consecutive dims of one cached token -> fp16, natural order.  KV4: `w0` holds the 8 nibbles; KV8: `w0`, `w1` the 8 bytes.
template <bool INT4>
__device__ __forceinline__ h8 dequant8(u32 w0, u32 w1, _Float16 sc, _Float16 zr) {
    const float scf = (float)sc, zrf = (float)zr;
    if (INT4) {
        const _Float16 hz = (_Float16)(-scf * zrf);
        const h2 vs = {sc, sc}, vz = {hz, hz};
        h2 e[4];
        nib8_to_h2(w0, e);
#pragma unroll
        for (int r = 0; r < 4; ++r) e[r] = __builtin_elementwise_fma(e[r], vs, vz);
        return (h8){e[0][0], e[1][0], e[2][0], e[3][0], e[0][1], e[1][1], e[2][1], e[3][1]};
    }
    h8 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        o[j] = (_Float16)(scf * ((float)((w0 >> (8 * j)) & 0xFFu) - zrf));
        o[4 + j] = (_Float16)(scf * ((float)((w1 >> (8 * j)) & 0xFFu) - zrf));
    }
    return o;
}

// Geometry of a launch - the ONE statement of it (the plan entries and the launchers all ask here).
struct AppendPlan {
    int tile_tokens, q_tiles, waves;
};
inline AppendPlan plan_append(int max_seqlen_q, int num_heads, int num_kv_heads) {
    const int G = num_heads / num_kv_heads;
    AppendPlan p;
    p.waves = NWV;
    p.tile_tokens = BM / G;          // rows = (token, head-in-group): every head of the group rides on the same staged tiles
    p.q_tiles = (max_seqlen_q + p.tile_tokens - 1) / p.tile_tokens;
    return p;
}

// The layout contract of the attention entries (include/qserve_amd.h), checked before any device call - the ONE statement of it
// (qs_append_attention and qs_append_attention_split both ask here; the group size is checked by the plan entries).
inline int check_append_args(const void* qkv, const void* out, const int32_t* cu_seqlens_q, const int32_t* past_lens,
                             const int64_t* kv_pointers, int num_tokens, int batch, int max_seqlen_q, int max_blocks, int num_heads,
                             int num_kv_heads, int head_dim, int64_t qkv_stride0, int64_t out_stride0, int tokens_per_block,
                             int size_per_token, int int4_kv_cache, int kv_cache_with_zeros) {
    QS_REQUIRE(qkv && out && cu_seqlens_q && past_lens && kv_pointers, "append_attention: null pointer");
    QS_REQUIRE(num_tokens >= 0 && batch >= 0 && max_seqlen_q >= 0 && max_blocks > 0, "append_attention: bad sizes");
    QS_REQUIRE(num_heads > 0 && num_kv_heads > 0 && num_heads % num_kv_heads == 0,
               "append_attention: bad head counts H=%d Hkv=%d", num_heads, num_kv_heads);
    if (head_dim != DH || tokens_per_block != BN || !kv_cache_with_zeros) {
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
    return QS_OK;
}

}  // namespace qs_append
