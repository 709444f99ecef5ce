// kv_commit.h -- the path-commit rule of tree-draft verification, shared by its two kernels: kv_commit_path_kernel (append_tree.hip, one
// layer per launch) and kv_commit_path_layers_kernel (tree_accept.hip, every layer in one launch).  DESIGN.md 10 ("Tree verification").
//
// One workgroup owns a (sequence, KV head, K | V) of ONE layer and calls commit_path_moves once.  Slot past + k receives the bytes - data,
// fp16 scale, fp16 zero - of slot past + idx[k], k < m.  A page: data [Hkv][64][DHB], then fp16 scales [Hkv][64], then fp16 zeros [Hkv][64];
// DHB = bytes per cached token and head (64 KV4, 128 KV8).  Move k: thread (k, c) of the data pass copies the 16-byte chunk c of the token,
// thread k of the parameter pass its scale and zero.  EVERY source is read into LDS, then a barrier, then the stores - a source may be
// another move's destination.  Identity moves are skipped; a move whose source or destination lies beyond the pointer table, or whose index
// is not in 0 .. 63, is dropped; nothing else in a page is written.  Vector stores only.
#pragma once
#include "common.h"

namespace qs_commit {

constexpr int SLOTS = 64;        // tokens per KV page
constexpr int MAX_PATH = 64;     // nodes per accepted path (= nodes per tree)

// tab: the (sequence, K | V) row of the layer's pointer table [max_blocks]; idx: the sequence's accept_idx row; m: its accept_len, already
// cut to 0 .. max_accept <= MAX_PATH.  s_data [MAX_PATH * DHB / 16] and s_par [MAX_PATH] are the workgroup's LDS.
template <int DHB>
__device__ __forceinline__ void commit_path_moves(const int64_t* __restrict__ tab, const int* __restrict__ idx, int m, int past, int hkv,
                                                  int max_blocks, int kv_head_num, v4u* s_data, u32* s_par) {
    constexpr int CH = DHB / 16;                         // 16-byte chunks per token
    const size_t par_off = (size_t)kv_head_num * SLOTS * DHB;   // the scales behind the data, the zeros kv_head_num * 64 fp16 further
    auto moves = [&](int k, int& src, int& dst) {               // -> does move k change anything?
        const int i = idx[k];
        src = past + i, dst = past + k;
        return i != k && i >= 0 && i < MAX_PATH && past >= 0 && src < max_blocks * SLOTS && dst < max_blocks * SLOTS;
    };
    auto token = [&](int pos) { return reinterpret_cast<uint8_t*>(tab[pos >> 6]) + ((size_t)hkv * SLOTS + (pos & 63)) * DHB; };
    auto param = [&](int pos) {
        return reinterpret_cast<uint16_t*>(reinterpret_cast<uint8_t*>(tab[pos >> 6]) + par_off) + hkv * SLOTS + (pos & 63);
    };
    int src, dst;
    for (int j = threadIdx.x; j < m * CH; j += blockDim.x)
        if (moves(j / CH, src, dst)) s_data[j] = *reinterpret_cast<const v4u*>(token(src) + (j % CH) * 16);
    for (int k = threadIdx.x; k < m; k += blockDim.x)
        if (moves(k, src, dst)) {
            const uint16_t* p = param(src);
            s_par[k] = (u32)p[0] | ((u32)p[kv_head_num * SLOTS] << 16);
        }
    __syncthreads();                                     // every source is read (its data sits in LDS) before any destination is written
    for (int j = threadIdx.x; j < m * CH; j += blockDim.x)
        if (moves(j / CH, src, dst)) *reinterpret_cast<v4u*>(token(dst) + (j % CH) * 16) = s_data[j];
    for (int k = threadIdx.x; k < m; k += blockDim.x)
        if (moves(k, src, dst)) {
            uint16_t* p = param(dst);
            p[0] = (uint16_t)(s_par[k] & 0xFFFFu);
            p[kv_head_num * SLOTS] = (uint16_t)(s_par[k] >> 16);
        }
}

}  // namespace qs_commit
