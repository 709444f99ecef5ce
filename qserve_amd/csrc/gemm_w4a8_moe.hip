// gemm_w4a8_moe.hip -- grouped W4A8 GEMM for mixture-of-experts layers (no reference counterpart: the reference's
// MoEW4A8OF16LinearDynamicInputScale.forward raises "MOE implementation is yet to be released").
//
//   out[p, :] = W[e] x[row_src[p], :]   for every sorted position p, e = the expert whose range expert_offsets[e] <= p <
//   expert_offsets[e + 1] holds p;  row_src == nullptr: x row p.
//
// Weights: the reference's packed layout (gemm_w4a8.hip header) stacked over experts and consumed as is - qweight [E, N, K/2],
// s1_scales / s1_szeros [E, N], per-group s2_zeros / s2_scales [E, K/128, N].  The activation scales (and row sums) belong to the
// SOURCE row.  Arithmetic of the dense entries: the MFMA mapping, exact int32 accumulation and the epilogues of common.h, so the output
// of a pair equals, bit for bit, what qs_w4a8_per_chn_gemm / qs_w4a8_per_group_gemm give for that expert's weights on that row.
//
// Kernel `w4a8_moe_gemm`, modelled on w4a8_gemm_splitk (gemm_w4a8.hip): a workgroup owns (expert, 64-channel unit, block of 16 MT
// sorted rows); its NW waves take the k-steps round-robin and reduce through LDS.  grid = (N / 64, row blocks); the row blocks are the
// host-known bound of moe_plan.h, ceil(P / (16 MT)) + E - 1, and a block finds its (expert, first row) from expert_offsets itself: lane
// e of every wave holds expert e (E <= 64), a wave prefix sum of the experts' block counts gives each its first block, and the one
// lane whose block range holds blockIdx.y names the expert.  Surplus blocks leave at once; rows of a block beyond its expert's range
// are computed on a clamped source row and not stored.  No cross-workgroup K split: (N / 64) x E workgroups fill the chip at the
// expert shapes, and without it there is no slab, counter or wait.  Activation rows are gathered through the per-lane row pointers.
// Index hygiene: offsets are clamped into [0, P] and a range that runs backwards is empty; row_src values are clamped into
// [0, x_rows - 1]: no device input moves an access outside the stated extents.
#include "common.h"
#include "moe_plan.h"
#include "gemm_plan.h"

namespace {

template <int MT>
struct MoeStage {
    v4u w[4];
    v4i b[MT][2];
    u32 sdw, zdw;
};

// MODE 0 = per-channel, 1 = per-group(128)
template <int MT, int MODE, int NSTAGE>
__global__ __launch_bounds__(MT <= 2 ? 512 : 256, 2) void w4a8_moe_gemm(
    const int8_t* __restrict__ X, long long x_stride, int x_rows, const int* __restrict__ row_src, const int* __restrict__ offsets,
    const uint8_t* __restrict__ Wall, const int8_t* __restrict__ zeros_all, const int8_t* __restrict__ scales8_all,
    const __half* __restrict__ wscales_all, const __half* __restrict__ ascales, const __half* __restrict__ wszs_all,
    const __half* __restrict__ assums, _Float16* __restrict__ out, long long out_stride, int P, int E, int N, int K, int epi_fma) {
    extern __shared__ __attribute__((aligned(16))) int red[];   // [NW][MT*16][64]
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int NW = blockDim.x >> 6;
    const int li = lane & 15, g = lane >> 4;
    const int tsel = li >> 3, c = li & 7;
    constexpr int R = 16 * MT;

    // ---- (expert, first row) of this row block, from the offsets: every wave does the same search (all 64 lanes active)
    int lo = 0, hi = 0;
    if (lane < E) {
        lo = offsets[lane], hi = offsets[lane + 1];
        lo = lo < 0 ? 0 : lo > P ? P : lo;
        hi = hi < 0 ? 0 : hi > P ? P : hi;
    }
    const int nblk = hi > lo ? (hi - lo + R - 1) / R : 0;
    int incl = nblk;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    const int first = incl - nblk;
    const int b = blockIdx.y;
    const unsigned long long owner = __ballot(nblk > 0 && b >= first && b < incl);
    if (owner == 0) return;                                        // surplus block (workgroup-uniform)
    const int e = __builtin_amdgcn_readfirstlane(__ffsll((long long)owner) - 1);
    const int row0 = __builtin_amdgcn_readlane(lo, e) + (b - __builtin_amdgcn_readlane(first, e)) * R;
    const int row_end = __builtin_amdgcn_readlane(hi, e);          // row0 < row_end <= P

    const int unit = blockIdx.x;
    const int T0 = unit * 2;
    const int KT = K >> 5;
    const int nsteps = K >> 7;
    const uint8_t* W = Wall + (size_t)e * N * (size_t)(K >> 1);
    const uint8_t* wrow = W + ((size_t)(T0 + tsel) * KT) * 512 + c * 64 + (size_t)g * 512;
    const int8_t* arow[MT];
    int src[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        int p = row0 + 16 * mt + li;
        p = p < row_end ? p : row_end - 1;
        int s = row_src ? row_src[p] : p;
        s = s < 0 ? 0 : s >= x_rows ? x_rows - 1 : s;
        src[mt] = s;
        arow[mt] = X + (size_t)s * (size_t)x_stride + 32 * g;
    }
    const int meta_off = (T0 + tsel) * 32 + c * 4;   // per-group scale / zero dword of this lane's 4 row classes
    const int8_t* zeros = MODE == 1 ? zeros_all + (size_t)e * nsteps * N : nullptr;
    const int8_t* scales8 = MODE == 1 ? scales8_all + (size_t)e * nsteps * N : nullptr;

    v4i acc[MT][4];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int cl = 0; cl < 4; ++cl) acc[mt][cl] = (v4i){0, 0, 0, 0};

    auto load_stage = [&](MoeStage<MT>& st, int ks) {
        const v4u* wp = reinterpret_cast<const v4u*>(wrow + (size_t)ks * 2048);
#pragma unroll
        for (int q = 0; q < 4; ++q) st.w[q] = wp[q];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const v4i* ap = reinterpret_cast<const v4i*>(arow[mt] + (size_t)ks * 128);
            st.b[mt][0] = ap[0];
            st.b[mt][1] = ap[1];
        }
        if (MODE == 1) {
            st.sdw = *reinterpret_cast<const u32*>(scales8 + (size_t)ks * N + meta_off);
            st.zdw = *reinterpret_cast<const u32*>(zeros + (size_t)ks * N + meta_off);
        }
    };
    auto compute_stage = [&](const MoeStage<MT>& st) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            u32 rx[4], ry[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                rx[q] = h ? st.w[q].z : st.w[q].x;
                ry[q] = h ? st.w[q].w : st.w[q].y;
            }
#pragma unroll
            for (int cl = 0; cl < 4; ++cl) {
                u32 s = 0, zb = 0;
                if (MODE == 1) {
                    s = (st.sdw >> (8 * cl)) & 0xFFu;
                    zb = ((st.zdw >> (8 * cl)) & 0xFFu) * 0x01010101u;
                }
                v4i a;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const u32 raw = (cl & 1) ? ry[q] : rx[q];
                    a[q] = (int)((cl & 2) ? unpack_hi<MODE>(raw, s, zb) : unpack_lo<MODE>(raw, s, zb));
                }
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
                    acc[mt][cl] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, st.b[mt][h], acc[mt][cl], 0, 0, 0);
            }
        }
    };

    // the waves take the k-steps round-robin, NSTAGE of a wave's steps in flight in registers (a wave beyond the steps adds zeros)
    MoeStage<MT> st[NSTAGE];
#pragma unroll
    for (int s = 0; s < NSTAGE; ++s) {
        const int kk = wave + s * NW;
        if (kk < nsteps) load_stage(st[s], kk);
    }
    for (int ks = wave; ks < nsteps; ks += NW * NSTAGE) {
#pragma unroll
        for (int s = 0; s < NSTAGE; ++s) {
            const int kk = ks + s * NW;
            if (kk < nsteps) {
                compute_stage(st[s]);
                const int nk = kk + NSTAGE * NW;
                if (nk < nsteps) load_stage(st[s], nk);
            }
        }
    }

    // ---- cross-wave reduction through LDS (int32: exact in any order); wave w finalises pairs p = w, w + NW, ...
    constexpr int NP = MT * 4;
    if (NW > 1) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int cl = 0; cl < 4; ++cl)
#pragma unroll
                for (int r = 0; r < 4; ++r) red[(wave * NP * 4 + (mt * 4 + cl) * 4 + r) * 64 + lane] = acc[mt][cl][r];
        __syncthreads();
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int cl = 0; cl < 4; ++cl) {
                const int p = mt * 4 + cl;
                if ((p % NW) != wave) continue;
                v4i s = (v4i){0, 0, 0, 0};
                for (int w = 0; w < NW; ++w)
#pragma unroll
                    for (int r = 0; r < 4; ++r) s[r] += red[(w * NP * 4 + p * 4 + r) * 64 + lane];
                acc[mt][cl] = s;
            }
    }

    // ---- epilogue: the dense entries' (common.h), scales of the expert's channels and of the SOURCE row
    const _Float16* wscales = reinterpret_cast<const _Float16*>(wscales_all) + (size_t)e * N;
    const _Float16* wszs = MODE == 0 ? reinterpret_cast<const _Float16*>(wszs_all) + (size_t)e * N : nullptr;
    const int ncol0 = 32 * (T0 + (g >> 1)) + 4 * (g & 1);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
        for (int cl = 0; cl < 4; ++cl) {
            const int p = mt * 4 + cl;
            if (NW > 1 && (p % NW) != wave) continue;
            const v4i s = acc[mt][cl];
            const int m = row0 + 16 * mt + li;
            const int n = ncol0 + 8 * cl;
            if (m < row_end) {
                h4 o;
                const float sa = __half2float(ascales[src[mt]]);
                const h4 ws4 = *reinterpret_cast<const h4*>(wscales + n);
                if (MODE == 0) {
                    const float ss = __half2float(assums[src[mt]]);
                    const h4 wz4 = *reinterpret_cast<const h4*>(wszs + n);
#pragma unroll
                    for (int r = 0; r < 4; ++r) o[r] = (_Float16)epi_per_chn(s[r], (float)ws4[r], sa, (float)wz4[r], ss, epi_fma);
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) o[r] = (_Float16)epi_per_group(s[r], (float)ws4[r], sa);
                }
                *reinterpret_cast<h4*>(out + (size_t)m * (size_t)out_stride + n) = o;
            }
        }
    }
}

struct MoeArgs {
    const int8_t* x;
    int64_t x_stride;
    int x_rows;
    const int32_t *row_src, *offsets;
    const int8_t *qweight, *zeros, *scales8;
    const void *wscales, *ascales, *wszs, *assums;
    void* out;
    int64_t out_stride;
    int P, E, N, K;
    hipStream_t stream;
};

template <int MT, int MODE>
int launch_moe(const MoeArgs& a, const moe_plan::MoePlan& pl) {
    auto kern = w4a8_moe_gemm<MT, MODE, 2>;
    const size_t smem = pl.nw > 1 ? (size_t)pl.nw * MT * 16 * 64 * sizeof(int) : 16;
    static size_t configured_dev[QS_MAX_DEVICES] = {};   // per instantiation and device (the reservation grows with the waves)
    size_t& configured = configured_dev[qs_device_slot()];
    if (smem > configured) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (e != hipSuccess) {
            qs_set_error("w4a8 moe gemm: cannot reserve %zu bytes of LDS: %s", smem, hipGetErrorString(e));
            return (int)e;
        }
        configured = smem;
    }
    hipLaunchKernelGGL(kern, dim3(pl.units, pl.mblocks), dim3(pl.nw * 64), smem, a.stream, a.x, (long long)a.x_stride, a.x_rows, a.row_src,
                       a.offsets, reinterpret_cast<const uint8_t*>(a.qweight), a.zeros, a.scales8, reinterpret_cast<const __half*>(a.wscales),
                       reinterpret_cast<const __half*>(a.ascales), reinterpret_cast<const __half*>(a.wszs),
                       reinterpret_cast<const __half*>(a.assums), reinterpret_cast<_Float16*>(a.out), (long long)a.out_stride, a.P, a.E, a.N,
                       a.K, (int)g_epi_fma);
    return qs_launch_status("w4a8 moe gemm");
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

int require_moe_shape(int P, int E, int N, int K) {
    QS_REQUIRE(P >= 0 && P <= (1 << 21), "w4a8 moe gemm: P=%d sorted rows (0 .. 2^21)", P);
    QS_REQUIRE(E >= 1 && E <= 64, "w4a8 moe gemm: E=%d experts (1 .. 64)", E);
    const gemm_plan::ShapeFault f = gemm_plan::check_shape(P, N, K);
    QS_REQUIRE(f != gemm_plan::SHAPE_BAD, "w4a8 moe gemm: bad shape P=%d N=%d K=%d", P, N, K);
    QS_REQUIRE(f != gemm_plan::SHAPE_N_NOT_64, "w4a8 moe gemm: N=%d must be a multiple of 64", N);
    QS_REQUIRE(f != gemm_plan::SHAPE_K_NOT_128, "w4a8 moe gemm: K=%d must be a multiple of 128", K);
    QS_REQUIRE(N <= (1 << 22) && K <= (1 << 20), "w4a8 moe gemm: N=%d (<= 2^22), K=%d (<= 2^20)", N, K);
    return QS_OK;
}

template <int MODE>
int moe_gemm(const MoeArgs& a) {
    if (int rc = require_moe_shape(a.P, a.E, a.N, a.K)) return rc;
    QS_REQUIRE(a.x && a.offsets && a.qweight && a.wscales && a.ascales && a.out, "w4a8 moe gemm: null pointer");
    if (MODE == 0) QS_REQUIRE(a.wszs && a.assums, "w4a8 per-channel moe gemm: null w_szs / a_ssums");
    if (MODE == 1) QS_REQUIRE(a.zeros && a.scales8, "w4a8 per-group moe gemm: null zeros / scales_i8");
    QS_REQUIRE(a.x_stride >= a.K && a.x_stride % 16 == 0 && a.out_stride >= a.N && a.out_stride % 8 == 0,
               "w4a8 moe gemm: x stride %lld (>= K=%d, a multiple of 16), out stride %lld (>= N=%d, a multiple of 8)", (long long)a.x_stride,
               a.K, (long long)a.out_stride, a.N);
    QS_REQUIRE(a.x_rows >= 1 && a.x_rows <= (1 << 24) && (a.row_src || a.x_rows >= a.P),
               "w4a8 moe gemm: x_rows=%d (1 .. 2^24; without row_src at least P=%d)", a.x_rows, a.P);
    QS_REQUIRE(aligned(a.x, 16) && aligned(a.qweight, 16) && aligned(a.out, 16) && aligned(a.wscales, 8) && aligned(a.wszs, 8) &&
                   aligned(a.zeros, 4) && aligned(a.scales8, 4) && aligned(a.offsets, 4) && aligned(a.row_src, 4) && aligned(a.ascales, 2) &&
                   aligned(a.assums, 2),
               "w4a8 moe gemm: x, qweight and out must be 16-byte, the weight scales 8-byte, the level-2 scales / zeros, the offsets and "
               "row_src 4-byte, the activation scales 2-byte aligned");
    if (a.P == 0) return QS_OK;
    const moe_plan::MoePlan pl = moe_plan::plan_moe(a.P, a.E, a.N, a.K);
    switch (pl.mt) {
    case 1: return launch_moe<1, MODE>(a, pl);
    case 2: return launch_moe<2, MODE>(a, pl);
    default: return launch_moe<4, MODE>(a, pl);
    }
}

}  // namespace

extern "C" int qs_moe_gemm_plan(int P, int E, int N, int K, int* plan4) {
    QS_REQUIRE(plan4, "moe gemm plan: null output");
    for (int i = 0; i < 4; ++i) plan4[i] = 0;
    if (int rc = require_moe_shape(P, E, N, K)) return rc;
    const moe_plan::MoePlan pl = moe_plan::plan_moe(P, E, N, K);
    plan4[0] = pl.mt, plan4[1] = pl.nw, plan4[2] = pl.mblocks, plan4[3] = pl.units;
    return QS_OK;
}

extern "C" int qs_w4a8_per_chn_moe_gemm(const int8_t* x, int64_t x_stride, int x_rows, const int32_t* row_src, const int32_t* expert_offsets,
                                        const int8_t* qweight, const void* wscales, const void* ascales, const void* w_szs,
                                        const void* a_ssums, void* out, int64_t out_stride, int P, int E, int N, int K, qs_stream_t stream) {
    MoeArgs a = {x, x_stride, x_rows, row_src, expert_offsets, qweight, nullptr, nullptr, wscales, ascales, w_szs, a_ssums, out, out_stride,
                 P, E, N, K, reinterpret_cast<hipStream_t>(stream)};
    return moe_gemm<0>(a);
}

extern "C" int qs_w4a8_per_group_moe_gemm(const int8_t* x, int64_t x_stride, int x_rows, const int32_t* row_src,
                                          const int32_t* expert_offsets, const int8_t* qweight, const int8_t* zeros, const int8_t* scales_i8,
                                          const void* wscales, const void* ascales, void* out, int64_t out_stride, int P, int E, int N, int K,
                                          qs_stream_t stream) {
    MoeArgs a = {x, x_stride, x_rows, row_src, expert_offsets, qweight, zeros, scales_i8, wscales, ascales, nullptr, nullptr, out, out_stride,
                 P, E, N, K, reinterpret_cast<hipStream_t>(stream)};
    return moe_gemm<1>(a);
}
