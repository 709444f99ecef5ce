// attention_long_walk.h -- what attention_long.hip (every cached page) and attention_window.hip (the pages of a sliding window) share
// around the workgroup's statements (attention_long_body.h): the LDS layout, the wave quantiser of the new token, the entries'
// argument contract and the launch of a KV4 / KV8 kernel pair.  The comments on mapping, data movement and arithmetic stand in
// attention_long.hip, once.
#pragma once
#include "append_dequant.h"
#include "attn_host.h"
#include "kv_quant.h"

namespace qs_long {

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

// ---- host side: the two entries' argument contract, checked before any device call, and the launch of a kernel pair -------------
inline int check_decode_long_args(const char* what, const void* q, const void* k, const void* v, const int64_t* kv_pointers,
                                  const int32_t* length_per_sample, void* out, int batch, int num_heads, int num_kv_heads, int head_dim,
                                  int64_t q_stride0, int64_t kv_stride0, int max_blocks, int memory_max_seqlen, int tokens_per_block,
                                  int size_per_token, int timestep, int rotary_embedding_dim, float rotary_base, int int4_kv_cache,
                                  int kv_cache_with_zeros, int num_splits, qs_stream_t stream, DecodeLongArgs* a) {
    QS_REQUIRE(q && k && v && kv_pointers && out, "%s: null pointer", what);
    QS_REQUIRE(batch >= 0 && num_heads > 0 && num_kv_heads > 0 && num_heads % num_kv_heads == 0, "%s: bad head counts H=%d Hkv=%d", what,
               num_heads, num_kv_heads);
    const int G = num_heads / num_kv_heads;
    if (head_dim != 128 || rotary_embedding_dim != 128 || tokens_per_block != 64 || !kv_cache_with_zeros || G > 8) {
        qs_set_error("%s: only head_dim=128, rotary_dim=128, tokens_per_block=64, zero-point KV caches and "
                     "num_heads/num_kv_heads in 1..8 are supported (H=%d Hkv=%d)", what, num_heads, num_kv_heads);
        return QS_ENOSUP;
    }
    const int dhb = int4_kv_cache ? 64 : 128;
    QS_REQUIRE(size_per_token == num_kv_heads * dhb, "%s: size_per_token=%d, expected %d", what, size_per_token, num_kv_heads * dhb);
    QS_REQUIRE(max_blocks > 0 && memory_max_seqlen > 0, "%s: bad max_blocks / memory_max_seqlen", what);
    QS_REQUIRE(num_splits >= 0, "%s: num_splits=%d (0 = choose, >= 1 = that many ranges)", what, num_splits);
    QS_REQUIRE(q_stride0 % 8 == 0 && kv_stride0 % 8 == 0 && q_stride0 >= (int64_t)num_heads * 128 && kv_stride0 >= (int64_t)num_kv_heads * 128,
               "%s: token strides must hold the token's heads and keep 16-byte alignment", what);
    QS_REQUIRE(((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(v) |
                 reinterpret_cast<uintptr_t>(out)) & 15) == 0,
               "%s: q, k, v and out must be 16-byte aligned", what);
    QS_REQUIRE(batch <= 65535 && num_kv_heads <= 65535, "%s: batch and num_kv_heads are grid dimensions (<= 65535)", what);
    a->int4 = int4_kv_cache != 0, a->batch = batch;
    DecodeArgs& d = a->d;
    d.G = G, d.grid = dim3(num_kv_heads, batch), d.st = (hipStream_t)stream;
    d.q = (const _Float16*)q, d.k = (const _Float16*)k, d.v = (const _Float16*)v, d.kvp = kv_pointers, d.len = length_per_sample;
    d.out = (_Float16*)out, d.H = num_heads, d.Hkv = num_kv_heads, d.qs = q_stride0, d.kvs = kv_stride0, d.mb = max_blocks;
    d.timestep = timestep, d.base = rotary_base, d.max_pos = memory_max_seqlen, d.quant = nullptr, d.fused = nullptr;
    return QS_OK;
}

// plan.splits ranges per (sequence, KV head) - fewer where the workspace holds fewer, one (no workspace, no merge) where it cannot be
// had; `extra`: what the pair takes behind the workspace (the window)
template <auto KV4, auto KV8, class... Extra>
int launch_long_kernels(const char* what, const DecodeLongArgs& a, const LongPlan& plan, Extra... extra) {
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
    const void* kern = a.int4 ? reinterpret_cast<const void*>(KV4) : reinterpret_cast<const void*>(KV8);
    if (const hipError_t e = qs_reserve_lds({kern}, bytes, a.int4 ? lds4 : lds8); e != hipSuccess) {
        qs_set_error("%s: cannot reserve %d bytes of LDS: %s", what, bytes, hipGetErrorString(e));
        return (int)e;
    }
    if (a.int4)
        hipLaunchKernelGGL(KV4, grid, dim3(TPB), bytes, st, q, k, v, kvp, len, out, H, Hkv, G, qs, kvs, mb, timestep, base, tab, tab_len, S,
                           plan.min_pages, ws, extra...);
    else
        hipLaunchKernelGGL(KV8, grid, dim3(TPB), bytes, st, q, k, v, kvp, len, out, H, Hkv, G, qs, kvs, mb, timestep, base, tab, tab_len, S,
                           plan.min_pages, ws, extra...);
    if (S > 1) qs_launch_attention_merge(ws, out, H, Hkv, G, S, a.batch, st);
    return qs_launch_status(what);
}

}  // namespace qs_long
