// sample_rows.hip -- the sampling head of the decode step and of sampled tree verification, for MI355X (gfx950): temperature, top-k and
// top-p over fp16 logit rows, one token per row, on the device.  DESIGN.md 10 ("Sampled verification"); the contract is in
// include/qserve_amd.h.  (Its own translation unit: the kernel sets of fused_small.hip and tree_accept.hip are checked contracts.)
// This file holds ONE kernel:
//
//   sample_rows_kernel  one workgroup of 1024 threads per row; the row (256 KB at n = 128 256) stays in L2 across the passes.  Every weight
//              w_i = exp((x_i - m) / T) is turned into the integer F_i = floor(w_i * 2^40) as soon as it is computed and EVERY sum below is
//              a sum of such integers: exact, independent of the order of the additions, hence bit-identical run to run and under graph
//              replay - no floating-point accumulation anywhere.  (w <= 1 and n <= 2^22, so a row's sum stays below 2^63; the
//              truncation costs n * 2^-40 <= 2^-18 of W >= 1.)
//                1. maximum and its first index (argmax_rows_kernel's rule).  Greedy rows end here.
//                2. only with top-k or top-p on: count and mass per coarse bin (the upper 10 bits of the order-preserving 16-bit key of an
//                   fp16 value) with LDS atomics, a descending workgroup scan finds the bin that holds each threshold; a second histogram
//                   over that bin's 64 values and a wave scan find the value itself.  Thresholds are VALUES: a tie class stays whole.
//                3. survivors' mass per wave segment (16 contiguous segments of the row, coalesced 16-byte loads), W_S, target =
//                   floor(u * W_S); the one wave whose segment holds the crossing walks it again 64 units at a time with a wave scan and
//                   the crossing lane walks its 8 elements: the smallest j with prefix(j) > target, the prefix in INDEX order.
//              The last 16-byte unit of a row may reach into the padding behind n (row_stride is a multiple of 8, so it stays inside the
//              row's stride): those elements are masked by index in every pass.  No scratch; 13.5 KB of LDS.
#include "common.h"

namespace {

typedef unsigned long long u64;
constexpr int TPB = 1024, WAVES = TPB / 64, COARSE = 1024, FINE = 64;
constexpr float FIX = 1099511627776.0f;                   // 2^40

// fp16 bits -> a 16-bit key that orders like the value (-0 is the value +0)
__device__ __forceinline__ u32 order_key(u32 b) {
    if (b == 0x8000u) b = 0;
    return b ^ ((b & 0x8000u) ? 0xFFFFu : 0x8000u);
}

__device__ __forceinline__ u64 fixed_weight(float x, float m, float scale) {
    float w = __builtin_amdgcn_exp2f((x - m) * scale);
    w = w >= 0.f ? (w <= 1.f ? w : 1.f) : 0.f;            // (NaN - a bad row - counts as 0)
    return (u64)(w * FIX);
}

__device__ __forceinline__ u64 wave_scan(u64 v, int lane) {   // inclusive
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u64 o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}

// inclusive scan over the workgroup in thread order; s_w: WAVES words
__device__ __forceinline__ u64 block_scan(u64 v, u64* s_w, int lane, int wave) {
    const u64 inc = wave_scan(v, lane);
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    u64 off = 0;
    for (int w = 0; w < wave; ++w) off += s_w[w];
    __syncthreads();
    return inc + off;
}

// the eight fixed-point weights of 16-byte unit `unit` (0 for an element behind n or below the threshold) -> their sum
__device__ __forceinline__ u64 unit_weights(const _Float16* row, int unit, int n, float m, float scale, u32 thr, u64 (&F)[8]) {
    const h8 v = *reinterpret_cast<const h8*>(row + (size_t)unit * 8);
    const v4u bits = __builtin_bit_cast(v4u, v);
    u64 sum = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const u32 b = (bits[e >> 1] >> ((e & 1) * 16)) & 0xFFFFu;
        const bool in = unit * 8 + e < n && order_key(b) >= thr;
        F[e] = in ? fixed_weight((float)v[e], m, scale) : 0;
        sum += F[e];
    }
    return sum;
}

// Philox4x32-10, first output word; counter (ctr_lo, ctr_hi, 0, 0), key (seed_lo, seed_hi)
__device__ __forceinline__ u32 philox_first(u64 ctr, u64 seed) {
    u32 c0 = (u32)ctr, c1 = (u32)(ctr >> 32), c2 = 0, c3 = 0, k0 = (u32)seed, k1 = (u32)(seed >> 32);
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const u64 p0 = (u64)0xD2511F53u * c0, p1 = (u64)0xCD9E8D57u * c2;
        const u32 n0 = (u32)(p1 >> 32) ^ c1 ^ k0, n2 = (u32)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0;
        c1 = (u32)p1;
        c2 = n2;
        c3 = (u32)p0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c0;
}

__device__ __forceinline__ void argmax_pick(float& bv, int& bi, float v, int i) {
    if (v > bv || (v == bv && i < bi)) {
        bv = v;
        bi = i;
    }
}

// grid = (rows), 1024 threads
__global__ __launch_bounds__(TPB) void sample_rows_kernel(const _Float16* __restrict__ x, int64_t* __restrict__ out, int n, int64_t row_stride,
                                                          float temperature, int top_k, float top_p, const float* __restrict__ row_t,
                                                          const int* __restrict__ row_k, const float* __restrict__ row_p,
                                                          const float* __restrict__ uniforms, u64 seed, const int64_t* __restrict__ row_keys,
                                                          float* __restrict__ u_out) {
    __shared__ u64 s_cmass[COARSE];
    __shared__ u32 s_ccnt[COARSE];
    __shared__ u64 s_fmass[FINE];
    __shared__ u32 s_fcnt[FINE];
    __shared__ u64 s_w[WAVES];
    __shared__ u64 s_above[3];                            // total mass | mass above the nucleus bin | count above the top-k bin
    __shared__ int s_bin[2];
    __shared__ u32 s_thr;
    __shared__ float s_v[WAVES];
    __shared__ int s_i[WAVES];
    __shared__ float s_u;
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const _Float16* row = x + (size_t)r * row_stride;
    const int units = (n + 7) >> 3;
    const float T = row_t ? row_t[r] : temperature, p = row_p ? row_p[r] : top_p;
    const int k = row_k ? row_k[r] : top_k;

    if (tid == 0) {                                       // the row's uniform
        float u;
        if (uniforms) u = uniforms[r];
        else u = (float)(philox_first(row_keys ? (u64)row_keys[r] : (u64)r, seed) >> 8) * 0x1p-24f;
        u = u >= 0.f ? (u <= 1.f - 0x1p-24f ? u : 1.f - 0x1p-24f) : 0.f;
        s_u = u;
        if (u_out) u_out[r] = u;
    }

    // ---- 1. the maximum and its first index
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int un = tid; un < units; un += TPB) {
        const h8 v = *reinterpret_cast<const h8*>(row + (size_t)un * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (un * 8 + e < n) argmax_pick(bv, bi, (float)v[e], un * 8 + e);
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const float ov = __shfl_xor(bv, s, 64);
        const int oi = __shfl_xor(bi, s, 64);
        argmax_pick(bv, bi, ov, oi);
    }
    if (lane == 0) {
        s_v[wave] = bv;
        s_i[wave] = bi;
    }
    __syncthreads();
    bv = s_v[0];
    bi = s_i[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) argmax_pick(bv, bi, s_v[w], s_i[w]);
    const float m = bv;
    const int amax = bi == 0x7fffffff ? 0 : bi;
    const float u = s_u;
    if (!(T >= 1e-5f) || !(p >= 1e-8f)) {                 // greedy (a NaN parameter too)
        if (tid == 0) out[r] = amax;
        return;
    }
    const float scale = (float)(1.4426950408889634 / (double)T);
    const bool k_on = k > 0 && k < n, p_on = p < 1.f;

    // ---- 2. the value threshold of the filters (key 0: everything survives)
    u32 thr = 0;
    if (k_on || p_on) {
        s_cmass[tid] = 0;
        s_ccnt[tid] = 0;
        if (tid < FINE) {
            s_fmass[tid] = 0;
            s_fcnt[tid] = 0;
        }
        if (tid < 2) s_bin[tid] = -1;
        __syncthreads();
        for (int un = tid; un < units; un += TPB) {
            const h8 v = *reinterpret_cast<const h8*>(row + (size_t)un * 8);
            const v4u bits = __builtin_bit_cast(v4u, v);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                if (un * 8 + e >= n) continue;
                const u32 bin = order_key((bits[e >> 1] >> ((e & 1) * 16)) & 0xFFFFu) >> 6;
                if (p_on) {
                    const u64 f = fixed_weight((float)v[e], m, scale);
                    if (f) atomicAdd(&s_cmass[bin], f);
                }
                if (k_on) atomicAdd(&s_ccnt[bin], 1u);
            }
        }
        __syncthreads();
        const int b = COARSE - 1 - tid;                   // descending: thread 0 owns the bin of the largest values
        const u64 mt = s_cmass[b], ct = s_ccnt[b];
        const u64 cum_m = block_scan(mt, s_w, lane, wave), cum_c = block_scan(ct, s_w, lane, wave);
        if (tid == TPB - 1) s_above[0] = cum_m;
        __syncthreads();
        const u64 W = s_above[0];
        u64 P = (u64)ceil((double)p * (double)W);         // tail mass >= p * W  <=>  tail mass >= P (integers)
        P = P < 1 ? 1 : P > W ? W : P;
        if (p_on && W > 0 && cum_m >= P && cum_m - mt < P) {
            s_bin[0] = b;
            s_above[1] = cum_m - mt;
        }
        if (k_on && cum_c >= (u64)k && cum_c - ct < (u64)k) {
            s_bin[1] = b;
            s_above[2] = cum_c - ct;
        }
        __syncthreads();
        const int bin_p = s_bin[0], bin_k = s_bin[1];
        for (int un = tid; un < units; un += TPB) {
            const h8 v = *reinterpret_cast<const h8*>(row + (size_t)un * 8);
            const v4u bits = __builtin_bit_cast(v4u, v);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                if (un * 8 + e >= n) continue;
                const u32 key = order_key((bits[e >> 1] >> ((e & 1) * 16)) & 0xFFFFu);
                const int bin = (int)(key >> 6);
                if (bin == bin_p) {
                    const u64 f = fixed_weight((float)v[e], m, scale);
                    if (f) atomicAdd(&s_fmass[key & (FINE - 1)], f);
                }
                if (bin == bin_k) atomicAdd(&s_fcnt[key & (FINE - 1)], 1u);
            }
        }
        __syncthreads();
        if (wave == 0) {
            const int c = FINE - 1 - lane;                // descending again
            u32 t = 0;
            if (bin_p >= 0) {
                const u64 cum = s_above[1] + wave_scan(s_fmass[c], lane);
                const u64 votes = __ballot(cum >= P);
                if (votes) t = ((u32)bin_p << 6) | (u32)(FINE - __ffsll(votes));
            }
            if (bin_k >= 0) {
                const u64 cum = s_above[2] + wave_scan((u64)s_fcnt[c], lane);
                const u64 votes = __ballot(cum >= (u64)k);
                if (votes) {
                    const u32 tk = ((u32)bin_k << 6) | (u32)(FINE - __ffsll(votes));
                    t = tk > t ? tk : t;
                }
            }
            if (lane == 0) s_thr = t;
        }
        __syncthreads();
        thr = s_thr;
    }

    // ---- 3. the draw: index-ordered prefix over the survivors
    const int seg = (units + WAVES - 1) / WAVES, lo = wave * seg, hi = lo + seg < units ? lo + seg : units;
    u64 F[8];
    u64 acc = 0;
    for (int un = lo + lane; un < hi; un += 64) acc += unit_weights(row, un, n, m, scale, thr, F);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) acc += __shfl_xor(acc, s, 64);
    if (lane == 0) s_w[wave] = acc;
    __syncthreads();
    u64 WS = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) WS += s_w[w];
    if (WS == 0) {                                        // a row without a finite logit: still an index in [0, n)
        if (tid == 0) out[r] = amax;
        return;
    }
    const u64 target = (u64)((double)u * (double)WS);     // prefix > u * W_S  <=>  prefix > floor(u * W_S)
    u64 before = 0, run = 0;                              // the mass in front of the wave whose segment holds the crossing
    int wsel = -1;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        if (wsel < 0 && target < run + s_w[w]) {
            wsel = w;
            before = run;
        }
        run += s_w[w];
    }
    if (wave != wsel) return;
    for (int base = lo; base < hi; base += 64) {          // (wave-uniform)
        const int un = base + lane;
        u64 s = 0;
        if (un < hi) s = unit_weights(row, un, n, m, scale, thr, F);
        const u64 inc = before + wave_scan(s, lane);
        const u64 votes = __ballot(inc > target);
        if (votes) {
            if (lane == __ffsll(votes) - 1) {
                u64 c = inc - s;
                int res = -1;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    c += F[e];
                    if (res < 0 && c > target) res = un * 8 + e;
                }
                out[r] = res;
            }
            return;
        }
        before = __shfl(inc, 63, 64);
    }
    if (lane == 0) out[r] = amax;                         // (not reached: the sums are exact and target < W_S)
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

extern "C" int qs_sample_rows(const void* logits, int64_t* out, int rows, int n, int64_t row_stride, float temperature, int top_k, float top_p,
                              const float* row_temperature, const int32_t* row_top_k, const float* row_top_p, const float* uniforms,
                              uint64_t seed, const int64_t* row_keys, float* u_out, qs_stream_t stream) {
    QS_REQUIRE(logits && out, "sample_rows: null pointer");
    QS_REQUIRE(n >= 8 && n <= (1 << 22) && row_stride >= n && row_stride % 8 == 0,
               "sample_rows: n=%d (8 .. 4194304), row stride %lld (must be >= n, multiple of 8)", n, (long long)row_stride);
    QS_REQUIRE(rows >= 0, "sample_rows: rows=%d", rows);
    QS_REQUIRE(aligned(logits, 16), "sample_rows: logits must be 16-byte aligned");
    QS_REQUIRE(aligned(out, 8) && aligned(row_keys, 8), "sample_rows: out and row_keys must be 8-byte aligned");
    QS_REQUIRE(aligned(row_temperature, 4) && aligned(row_top_k, 4) && aligned(row_top_p, 4) && aligned(uniforms, 4) && aligned(u_out, 4),
               "sample_rows: the per-row parameter arrays, uniforms and u_out must be 4-byte aligned");
    if (rows == 0) return QS_OK;
    hipLaunchKernelGGL(sample_rows_kernel, dim3(rows), dim3(TPB), 0, (hipStream_t)stream, (const _Float16*)logits, out, n, row_stride,
                       temperature, top_k, top_p, row_temperature, row_top_k, row_top_p, uniforms, (u64)seed, row_keys, u_out);
    return qs_launch_status("sample_rows");
}
