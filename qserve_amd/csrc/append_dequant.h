// append_dequant.h -- the leaves the append attention kernels (append_attention.hip, append_attention_split.hip, append_tree.hip)
// share: the exact KV4 / KV8 -> fp16 de-quantisation of 8 consecutive dims of a cached token (the decode kernels' values) and the
// scalar form of a page address for the LDS-DMA's base operand.  The page staging and the key loop built from these leaves are
// append_walk.h; the launch geometry is attn_plan.h's, the argument checks attn_host.h's.
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

}  // namespace qs_append
