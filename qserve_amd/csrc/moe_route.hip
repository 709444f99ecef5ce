// moe_route.hip -- the two row kernels around the grouped W4A8 GEMMs of a mixture-of-experts layer (gemm_w4a8_moe.hip); no reference
// counterpart: the reference's Mixtral block imports a `moe_helpers` that was never released.
//
// qs_moe_route: fp16 router logits [T, E] -> per token the k experts with the largest logits, ordered by (value descending, expert
// index ascending) on the fp16 values themselves; weights = softmax over the k chosen logits, op by op in float32:
//     e_j = expf(float(l_j) - float(l_0)),  s = ((e_0 + e_1) + ...) + e_{k-1},  w_j = e_j / s
// (the Mixtral rule: softmax over all experts, renormalised over the top k).  Then the STABLE sort of the T k pairs by expert: inside an
// expert pairs keep their (t, j) order.  expert_offsets [E + 1] = exclusive prefix of the experts' pair counts, pair_token [T k] = the
// source token of every sorted position, pair_pos [T, k] = the sorted position of every pair.  Deterministic: no atomic decides an
// output - counts come from ordered walks, one lane per expert.
//   * T <= 256 and T k <= 2048: ONE launch of one workgroup (the decode step's shape): selection, then the ids meet in LDS and the
//     first wave ranks them with one ballot per expert and 64-pair slice.
//   * otherwise four launches over chunks of 1024 pairs: select; per (chunk, expert) counts; one workgroup turns the counts into each
//     (chunk, expert)'s first position and writes the offsets; every chunk scatters its pairs in order.  The counts live in the
//     caller's workspace (qs_moe_route_workspace).
// Both paths compute the same integers and the same float operations per token.
//
// qs_moe_combine: out[t, :] = half(sum_j weights[t, j] * float(y[pair_pos[t, j], :])), float32, j ascending, the first product alone,
// multiply and add rounded separately (no contraction), one rounding to fp16.  pair_pos values are clamped into [0, T k - 1].
#include "common.h"

namespace {

constexpr int MR_MAX_E = 64, MR_MAX_K = 8;
constexpr int MR_CHUNK = 1024;            // pairs per chunk of the multi-launch path
constexpr int MR_SMALL_T = 256, MR_SMALL_PAIRS = 2048;
constexpr int MR_MAX_T = 1 << 24;

// one token: its k experts and weights -> ids[0 .. k-1], w[0 .. k-1]
__device__ __forceinline__ void route_token(const _Float16* __restrict__ row, int E, int k, int* __restrict__ ids, float* __restrict__ w) {
    float lv[MR_MAX_K];
    int li[MR_MAX_K];
    float pv = 0.f;
    int pi = -1;
#pragma unroll
    for (int j = 0; j < MR_MAX_K; ++j) {
        if (j < k) {
            // the greatest remaining element: behind the previous pick in the order (value descending, index ascending)
            float bv = 0.f;
            int bi = -1;
            for (int i = 0; i < E; ++i) {
                const float v = (float)row[i];
                const bool open = pi < 0 || v < pv || (v == pv && i > pi);
                if (open && (bi < 0 || v > bv)) bv = v, bi = i;
            }
            lv[j] = bv, li[j] = bi;
            pv = bv, pi = bi;
        }
    }
    float ev[MR_MAX_K];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < MR_MAX_K; ++j) {
        if (j < k) {
            ev[j] = expf(__fsub_rn(lv[j], lv[0]));
            s = j == 0 ? ev[0] : __fadd_rn(s, ev[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < MR_MAX_K; ++j) {
        if (j < k) {
            ids[j] = li[j];
            w[j] = __fdiv_rn(ev[j], s);
        }
    }
}

// exclusive prefix over the 64 lanes of a wave (all active)
__device__ __forceinline__ int wave_exclusive_sum(int v, int lane) {
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    return incl - v;
}

// ---- T <= 256, T k <= 2048: everything in one workgroup of 256 threads
__global__ __launch_bounds__(256) void moe_route_small(const _Float16* __restrict__ logits, long long stride, int T, int E, int k,
                                                        int* __restrict__ expert_ids, float* __restrict__ weights, int* __restrict__ offsets,
                                                        int* __restrict__ pair_token, int* __restrict__ pair_pos) {
    __shared__ int s_ids[MR_SMALL_PAIRS];
    const int t = threadIdx.x;
    if (t < T) {
        int ids[MR_MAX_K];
        float w[MR_MAX_K];
        route_token(logits + (size_t)t * stride, E, k, ids, w);
#pragma unroll
        for (int j = 0; j < MR_MAX_K; ++j)
            if (j < k) {
                s_ids[t * k + j] = ids[j];
                expert_ids[t * k + j] = ids[j];
                weights[t * k + j] = w[j];
            }
    }
    __syncthreads();
    if (t >= 64) return;
    const int P = T * k;
    // The first wave sorts: lane l holds pair p0 + l of every 64-pair slice, and one ballot per expert gives lane e its count and every
    // pair its rank among the pairs of its expert - earlier slices, then lower lanes: the (t, j) order - without a serial walk.
    int cnt = 0;                                   // lane e: the pairs of expert e
    for (int p0 = 0; p0 < P; p0 += 64) {
        const int id = p0 + t < P ? s_ids[p0 + t] : -1;
        for (int e = 0; e < E; ++e) {
            const unsigned long long m = __ballot(id == e);
            if (t == e) cnt += __popcll(m);
        }
    }
    const int first = wave_exclusive_sum(cnt, t);
    if (t < E) offsets[t] = first;
    if (t == E - 1) offsets[E] = first + cnt;      // = P
    int next = first;                              // lane e: the next free position of expert e
    const unsigned long long below = (1ull << t) - 1ull;
    for (int p0 = 0; p0 < P; p0 += 64) {
        const int p = p0 + t;
        const int id = p < P ? s_ids[p] : -1;
        int pos = -1;
        for (int e = 0; e < E; ++e) {
            const unsigned long long m = __ballot(id == e);
            const int base = __builtin_amdgcn_readlane(next, e);
            if (id == e) pos = base + __popcll(m & below);
            if (t == e) next += __popcll(m);
        }
        if (pos >= 0) {
            pair_token[pos] = p / k;
            pair_pos[p] = pos;
        }
    }
}

// ---- the multi-launch path
__global__ __launch_bounds__(256) void moe_route_select(const _Float16* __restrict__ logits, long long stride, int T, int E, int k,
                                                         int* __restrict__ expert_ids, float* __restrict__ weights) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    int ids[MR_MAX_K];
    float w[MR_MAX_K];
    route_token(logits + (size_t)t * stride, E, k, ids, w);
#pragma unroll
    for (int j = 0; j < MR_MAX_K; ++j)
        if (j < k) {
            expert_ids[(size_t)t * k + j] = ids[j];
            weights[(size_t)t * k + j] = w[j];
        }
}
// counts[chunk][e] = pairs of chunk `chunk` on expert e; lane e walks the chunk (the lanes read the same id: one broadcast load)
__global__ __launch_bounds__(64) void moe_route_count(const int* __restrict__ expert_ids, int P, int E, int* __restrict__ counts) {
    const int e = threadIdx.x, p0 = blockIdx.x * MR_CHUNK;
    const int p1 = p0 + MR_CHUNK < P ? p0 + MR_CHUNK : P;
    int cnt = 0;
    for (int p = p0; p < p1; ++p) cnt += expert_ids[p] == e ? 1 : 0;
    if (e < E) counts[(size_t)blockIdx.x * E + e] = cnt;
}
// counts -> the first sorted position of every (chunk, expert), in place; the offsets
__global__ __launch_bounds__(64) void moe_route_scan(int* __restrict__ counts, int chunks, int E, int* __restrict__ offsets) {
    const int e = threadIdx.x;
    int total = 0;
    if (e < E)
        for (int c = 0; c < chunks; ++c) total += counts[(size_t)c * E + e];
    int pos = wave_exclusive_sum(total, e);
    if (e < E) offsets[e] = pos;
    if (e == E - 1) offsets[E] = pos + total;
    if (e < E)
        for (int c = 0; c < chunks; ++c) {
            const int n = counts[(size_t)c * E + e];
            counts[(size_t)c * E + e] = pos;
            pos += n;
        }
}
__global__ __launch_bounds__(64) void moe_route_scatter(const int* __restrict__ expert_ids, const int* __restrict__ first, int P, int E, int k,
                                                         int* __restrict__ pair_token, int* __restrict__ pair_pos) {
    const int e = threadIdx.x, p0 = blockIdx.x * MR_CHUNK;
    const int p1 = p0 + MR_CHUNK < P ? p0 + MR_CHUNK : P;
    if (e >= E) return;
    int pos = first[(size_t)blockIdx.x * E + e];
    for (int p = p0; p < p1; ++p)
        if (expert_ids[p] == e) {
            pair_token[pos] = p / k;
            pair_pos[p] = pos++;
        }
}

// ---- combine: one thread per (token, 8 channels)
__global__ __launch_bounds__(256) void moe_combine_kernel(_Float16* __restrict__ out, long long out_stride, const _Float16* __restrict__ y,
                                                           long long y_stride, const float* __restrict__ weights,
                                                           const int* __restrict__ pair_pos, int k, int N, int P) {
    const int t = blockIdx.x, n = (blockIdx.y * 256 + threadIdx.x) * 8;
    if (n >= N) return;
    float acc[8];
    for (int j = 0; j < k; ++j) {
        int p = pair_pos[(size_t)t * k + j];
        p = p < 0 ? 0 : p >= P ? P - 1 : p;
        const float w = weights[(size_t)t * k + j];
        const h8 v = *reinterpret_cast<const h8*>(y + (size_t)p * (size_t)y_stride + n);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
#pragma clang fp contract(off)   // plain operators under the pragma: the _rn intrinsics carry their own contract flags and fuse into an fma
            const float term = w * (float)v[i];
            acc[i] = j == 0 ? term : acc[i] + term;
        }
    }
    h8 o;
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = (_Float16)acc[i];
    *reinterpret_cast<h8*>(out + (size_t)t * (size_t)out_stride + n) = o;
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

int require_route_shape(const char* what, int T, int E, int k) {
    QS_REQUIRE(T >= 0 && T <= MR_MAX_T, "%s: T=%d (0 .. 2^24)", what, T);
    QS_REQUIRE(E >= 1 && E <= MR_MAX_E, "%s: E=%d experts (1 .. %d)", what, E, MR_MAX_E);
    QS_REQUIRE(k >= 1 && k <= MR_MAX_K && k <= E, "%s: k=%d (1 .. min(E=%d, %d))", what, k, E, MR_MAX_K);
    QS_REQUIRE((int64_t)T * k <= (1 << 24), "%s: T k = %lld pairs (<= 2^24)", what, (long long)T * k);
    return QS_OK;
}
inline bool small_path(int T, int k) { return T <= MR_SMALL_T && T * k <= MR_SMALL_PAIRS; }
inline int64_t route_workspace(int T, int E, int k) {
    if (small_path(T, k)) return 16;
    const int64_t chunks = ((int64_t)T * k + MR_CHUNK - 1) / MR_CHUNK;
    return chunks * E * (int64_t)sizeof(int);
}

}  // namespace

extern "C" int64_t qs_moe_route_workspace(int T, int E, int k) {
    if (int rc = require_route_shape("moe_route_workspace", T, E, k)) return rc;
    return route_workspace(T, E, k);
}

extern "C" int qs_moe_route(const void* logits, int64_t logits_stride, int T, int E, int k, int32_t* expert_ids, float* weights,
                            int32_t* expert_offsets, int32_t* pair_token, int32_t* pair_pos, void* workspace, int64_t workspace_size,
                            qs_stream_t stream) {
    if (int rc = require_route_shape("moe_route", T, E, k)) return rc;
    QS_REQUIRE(logits && expert_ids && weights && expert_offsets && pair_token && pair_pos && workspace, "moe_route: null pointer");
    QS_REQUIRE(logits_stride >= E, "moe_route: logits stride %lld (>= E=%d)", (long long)logits_stride, E);
    QS_REQUIRE(aligned(logits, 2) && aligned(expert_ids, 4) && aligned(weights, 4) && aligned(expert_offsets, 4) && aligned(pair_token, 4) &&
                   aligned(pair_pos, 4) && aligned(workspace, 4),
               "moe_route: logits must be 2-byte, every other tensor 4-byte aligned");
    QS_REQUIRE(workspace_size >= route_workspace(T, E, k), "moe_route: the workspace holds %lld bytes, %lld are needed",
               (long long)workspace_size, (long long)route_workspace(T, E, k));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const _Float16* lg = reinterpret_cast<const _Float16*>(logits);
    if (small_path(T, k)) {   // (T == 0 too: the offsets are written, all zero)
        hipLaunchKernelGGL(moe_route_small, dim3(1), dim3(256), 0, s, lg, (long long)logits_stride, T, E, k, expert_ids, weights, expert_offsets,
                           pair_token, pair_pos);
        return qs_launch_status("moe_route");
    }
    const int P = T * k, chunks = (P + MR_CHUNK - 1) / MR_CHUNK;
    int* counts = reinterpret_cast<int*>(workspace);
    hipLaunchKernelGGL(moe_route_select, dim3((T + 255) / 256), dim3(256), 0, s, lg, (long long)logits_stride, T, E, k, expert_ids, weights);
    int rc = qs_launch_status("moe_route (select)");
    if (rc != QS_OK) return rc;
    hipLaunchKernelGGL(moe_route_count, dim3(chunks), dim3(64), 0, s, expert_ids, P, E, counts);
    if ((rc = qs_launch_status("moe_route (count)")) != QS_OK) return rc;
    hipLaunchKernelGGL(moe_route_scan, dim3(1), dim3(64), 0, s, counts, chunks, E, expert_offsets);
    if ((rc = qs_launch_status("moe_route (scan)")) != QS_OK) return rc;
    hipLaunchKernelGGL(moe_route_scatter, dim3(chunks), dim3(64), 0, s, expert_ids, counts, P, E, k, pair_token, pair_pos);
    return qs_launch_status("moe_route (scatter)");
}

extern "C" int qs_moe_combine(void* out, int64_t out_stride, const void* y, int64_t y_stride, const float* weights, const int32_t* pair_pos,
                              int T, int k, int N, qs_stream_t stream) {
    QS_REQUIRE(T >= 0 && T <= MR_MAX_T, "moe_combine: T=%d (0 .. 2^24)", T);
    QS_REQUIRE(k >= 1 && k <= MR_MAX_K, "moe_combine: k=%d (1 .. %d)", k, MR_MAX_K);
    QS_REQUIRE(N >= 64 && N % 64 == 0 && N <= (1 << 22), "moe_combine: N=%d (a multiple of 64, 64 .. 2^22)", N);
    QS_REQUIRE(out && y && weights && pair_pos, "moe_combine: null pointer");
    QS_REQUIRE(out_stride >= N && out_stride % 8 == 0 && y_stride >= N && y_stride % 8 == 0,
               "moe_combine: out stride %lld and y stride %lld (>= N=%d, multiples of 8)", (long long)out_stride, (long long)y_stride, N);
    QS_REQUIRE(aligned(out, 16) && aligned(y, 16) && aligned(weights, 4) && aligned(pair_pos, 4),
               "moe_combine: out and y must be 16-byte, weights and pair_pos 4-byte aligned");
    if (T == 0) return QS_OK;
    hipLaunchKernelGGL(moe_combine_kernel, dim3(T, (N / 8 + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<_Float16*>(out), (long long)out_stride, reinterpret_cast<const _Float16*>(y), (long long)y_stride,
                       weights, pair_pos, k, N, T * k);
    return qs_launch_status("moe_combine");
}
