// gemm_w4a8.hip -- W4A8 GEMMs for MI355X (gfx950): int8 activations x uint4 weights -> int32 (MFMA) -> fp16.
//
// Replaces (behaviour, not code) the reference kernels
//   kernels/csrc/qgemm/w4a8_per_chn/gemm_cuda.cu:303-594   (per-channel; zero point folded into the epilogue)
//   kernels/csrc/qgemm/w4a8_per_group/gemm_cuda.cu:328-628 (per-group-128; level-2 dequant u4 -> s8 in registers)
// and consumes the reference's packed `qweight` layout as is (w4a8_linear.py:196-226):
//   bytes [N/32][K/32][lane 32][16];  lane = c*4+e;  byte t = d*8+b*4+f;
//   low nibble  = W[32*n32 + 8b + c      ][32*k32 + 16d + 4e + f]
//   high nibble = W[32*n32 + 8b + c + 16 ][ same ]
// i.e. the 64 contiguous bytes at tile*512 + c*64 hold, for the four rows {c, 8+c, 16+c, 24+c} of the tile, all
// 32 k of the tile; dword e of {bytes 0-3 | 4-7 | 8-11 | 12-15} of chunk e = k {4e..4e+3} (+16 for bytes 8-15) of
// rows {c | 8+c} (low nibble) and {16+c | 24+c} (high nibble).
//
// CDNA4 mapping (this is NOT the reference's mma.m16n8k32 lane scheme):
//   v_mfma_i32_16x16x64_i8:  D[i][j] += sum_k A[i][k] B[k][j];  lane l supplies A[i=l&15][16 k of group g=l>>4] and
//   B[same 16 k][j=l&15] and receives D[i=4g+r][j=l&15], r=0..3.
//   * A operand = WEIGHTS.  MFMA row i <-> (tile select tsel=i>>3, c=i&7) of a 64-row "unit" (two n32 tiles);
//     lane (i,g) owns the 64-byte c-row of tile (T0+tsel, k32 = 4*kstep+g).  From those 64 bytes it builds, with
//     AND / shift only, eight operands: 4 row classes (x-lo, y-lo, x-hi, y-hi = rows c, 8+c, 16+c, 24+c) x 2 k-halves
//     (bytes 0-7 / 8-15 of every chunk).  Operand byte p=4e+f <-> k = 32*k32 + 16h + p: 16 CONTIGUOUS k, so
//   * B operand = ACTIVATIONS: lane (m=l&15, g) needs act[m][128*kstep + 32g + 16h .. +16]: plain 16-byte loads,
//     16 rows x 128 contiguous bytes per instruction.
//   * one k-step = 128 k = exactly one quantisation group: per-group scales/zeros are one dword per lane per step.
//   * accumulator (mt, cls)[r] of lane (m,g) is out[m0+16mt+m][32*(T0+(g>>1)) + 8cls + 4(g&1) + r]: four
//     consecutive channels -> one 8-byte fp16x4 store.
//   Integer accumulation is exact, so any consistent k-permutation is legal; the one above needs no cross-lane
//   movement at all.
//
// Kernel `w4a8_gemm_splitk`: one workgroup = NW waves that all own the same 64 output channels and (16*MT) tokens and
// split K between them (k-steps interleaved); partial int32 tiles are reduced through LDS and the fp32 epilogue is
// fused.  This is the decode-shape kernel (M <= 128: weight-streaming, HBM-bound; every weight byte is read once).
// Host side (below the kernel): the split-K workspace; the dispatcher, which launches what the pure planner (gemm_plan.h) returns
// through the family launchers of gemm_w4a8.h; the extern "C" entries, which fill the one GemmArgs record all of these take.
#include "gemm_w4a8.h"
#include "gemm_plan.h"

using namespace gemm_plan;

namespace {


// MODE 0 = per-channel, 1 = per-group(128).  OUTK 0 = fp16 epilogue, 1 = raw int32 accumulators.
//
// Work decomposition: grid = (N/64, ceil(M/(16 MT)), S).  The S blocks of one output tile and the NW waves of each
// block split the K/128 k-steps: block z owns a contiguous range, its waves take the steps of that range
// round-robin.  Each wave keeps NSTAGE k-steps of operands in flight in registers (weights are streamed from HBM
// exactly once; with ~2 us of loaded-HBM latency the bytes in flight per CU decide the bandwidth).
// Reduction: waves -> LDS (int32, exact) ; blocks -> per-tile int32 slabs in a workspace + arrival counter, the last
// arriving block sums the slabs and runs the fused fp32 epilogue (agent-scope release / acquire, placement
// independent; counters are reset by the last arriver so the workspace is reusable without host work).
template <int MT>
struct Stage {
    v4u w[4];
    v4i b[MT][2];
    u32 sdw, zdw;
};

template <int MT, int MODE, int OUTK, int NSTAGE>
__global__ __launch_bounds__(MT <= 2 ? 512 : 256, 2) void w4a8_gemm_splitk(const int8_t* __restrict__ A, const uint8_t* __restrict__ W,
                                                        const int8_t* __restrict__ zeros,
                                                        const int8_t* __restrict__ scales8,
                                                        const __half* __restrict__ wscales,
                                                        const __half* __restrict__ ascales,
                                                        const __half* __restrict__ wszs,
                                                        const __half* __restrict__ assums, void* __restrict__ out,
                                                        int* __restrict__ slabs, unsigned* __restrict__ counters,
                                                        int M, int N, int K, int mblocks, int epi_fma) {
    extern __shared__ __attribute__((aligned(16))) int red[];   // [NW][MT*16][64] ; red[0] doubles as the "last" flag
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int NW = blockDim.x >> 6;
    const int li = lane & 15, g = lane >> 4;
    const int tsel = li >> 3, c = li & 7;
    // (unit, token block) of this workgroup.  mblocks > 0 selects the XCD-aware 1-D mapping used when M is split over
    // workgroups: the observed dispatch puts workgroup b on XCD b % 8, so the `mblocks` workgroups that stream the SAME
    // 64 channels are made adjacent on ONE XCD (b, b+8, b+16, ...) and the weights are fetched from HBM once and
    // served to the others by that XCD's L2.  Placement affects speed only, never results.
    int unit = blockIdx.x, mblk = blockIdx.y;
    if (mblocks > 0) {
        const int b = blockIdx.x, slot = b >> 3;
        mblk = slot % mblocks;
        unit = (slot / mblocks) * 8 + (b & 7);
    }
    const int T0 = unit * 2;
    const int m0 = mblk * (16 * MT);
    const int KT = K >> 5;
    const int nsteps_all = K >> 7;
    const int S = gridDim.z, z = blockIdx.z;
    const int ks_begin = (int)(((long)nsteps_all * z) / S), ks_end = (int)(((long)nsteps_all * (z + 1)) / S);

    const uint8_t* wrow = W + ((size_t)(T0 + tsel) * KT) * 512 + c * 64 + (size_t)g * 512;
    const int8_t* arow[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        int row = m0 + 16 * mt + li;
        row = row < M ? row : M - 1;
        arow[mt] = A + (size_t)row * K + 32 * g;
    }
    const int meta_off = (T0 + tsel) * 32 + c * 4;   // per-group scale / zero dword of this lane's 4 row classes

    v4i acc[MT][4];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int cl = 0; cl < 4; ++cl) acc[mt][cl] = (v4i){0, 0, 0, 0};

    auto load_stage = [&](Stage<MT>& st, int ks) {
        const v4u* wp = reinterpret_cast<const v4u*>(wrow + (size_t)ks * 2048);
#pragma unroll
        for (int e = 0; e < 4; ++e) st.w[e] = wp[e];
        // (nontemporal loads measured 1.6x SLOWER for this 64-byte-row pattern: scripts/microbench_wstream.hip P2)
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
    auto compute_stage = [&](const Stage<MT>& st) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            u32 rx[4], ry[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                rx[e] = h ? st.w[e].z : st.w[e].x;
                ry[e] = h ? st.w[e].w : st.w[e].y;
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
                for (int e = 0; e < 4; ++e) {
                    const u32 raw = (cl & 1) ? ry[e] : rx[e];
                    a[e] = (int)((cl & 2) ? unpack_hi<MODE>(raw, s, zb) : unpack_lo<MODE>(raw, s, zb));
                }
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
                    acc[mt][cl] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, st.b[mt][h], acc[mt][cl], 0, 0, 0);
            }
        }
    };

    Stage<MT> st[NSTAGE];
#pragma unroll
    for (int s = 0; s < NSTAGE; ++s) {
        const int kk = ks_begin + wave + s * NW;
        if (kk < ks_end) load_stage(st[s], kk);
    }
    for (int ks = ks_begin + wave; ks < ks_end; ks += NW * NSTAGE) {
#pragma unroll
        for (int s = 0; s < NSTAGE; ++s) {
            const int kk = ks + s * NW;
            if (kk < ks_end) {
                compute_stage(st[s]);
                const int nk = kk + NSTAGE * NW;
                if (nk < ks_end) load_stage(st[s], nk);
            }
        }
    }

    // ---- cross-wave (split-K) reduction through LDS; wave w finalises pairs p = w, w+NW, ...
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

    // ---- cross-block reduction: slabs + arrival ticket, last arriver finalises ---------------------------------
    if (S > 1) {
        const size_t tile = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
        v4i* slab = reinterpret_cast<v4i*>(slabs) + (tile * S) * (size_t)(NP * 64);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int cl = 0; cl < 4; ++cl) {
                const int p = mt * 4 + cl;
                if (NW > 1 && (p % NW) != wave) continue;
                slab[((size_t)z * NP + p) * 64 + lane] = acc[mt][cl];
            }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();   // also orders the LDS reads above before red[0] is reused as a flag
        if (tid == 0) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const unsigned t = __hip_atomic_fetch_add(counters + tile, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            red[0] = (t == (unsigned)(S - 1)) ? 1 : 0;
        }
        __syncthreads();
        if (red[0] == 0) return;
        if (tid == 0) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            __hip_atomic_store(counters + tile, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // self-cleaning
        }
        __syncthreads();
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int cl = 0; cl < 4; ++cl) {
                const int p = mt * 4 + cl;
                if (NW > 1 && (p % NW) != wave) continue;
                v4i s = (v4i){0, 0, 0, 0};
                for (int zz = 0; zz < S; ++zz) {
                    const v4i t = slab[((size_t)zz * NP + p) * 64 + lane];
                    s += t;
                }
                acc[mt][cl] = s;
            }
    }

    // ---- fused epilogue -----------------------------------------------------------------------------------------
    const int ncol0 = 32 * (T0 + (g >> 1)) + 4 * (g & 1);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
        for (int cl = 0; cl < 4; ++cl) {
            const int p = mt * 4 + cl;
            if (NW > 1 && (p % NW) != wave) continue;
            const v4i s = acc[mt][cl];
            const int m = m0 + 16 * mt + li;
            const int n = ncol0 + 8 * cl;
            if (m < M) {
                if (OUTK == 1) {
                    *reinterpret_cast<v4i*>(reinterpret_cast<int*>(out) + (size_t)m * N + n) = s;
                } else {
                    h4 o;
                    const float sa = __half2float(ascales[m]);
                    const h4 ws4 = *reinterpret_cast<const h4*>(reinterpret_cast<const _Float16*>(wscales) + n);
                    if (MODE == 0) {
                        const float ss = __half2float(assums[m]);
                        const h4 wz4 = *reinterpret_cast<const h4*>(reinterpret_cast<const _Float16*>(wszs) + n);
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            o[r] = (_Float16)epi_per_chn(s[r], (float)ws4[r], sa, (float)wz4[r], ss, epi_fma);
                    } else {
#pragma unroll
                        for (int r = 0; r < 4; ++r) o[r] = (_Float16)epi_per_group(s[r], (float)ws4[r], sa);
                    }
                    *reinterpret_cast<h4*>(reinterpret_cast<_Float16*>(out) + (size_t)m * N + n) = o;
                }
            }
        }
    }
}

qs_flag g_variant = QS_GEMM_DEFAULT;   // process-global test / measurement hook (include/qserve_amd.h qs_gemm_variant_code): not thread-safe

// Split-K workspace (per device): int32 slabs + arrival counters, allocated lazily on first use (never while a
// stream is being captured: a failed allocation simply disables cross-block split-K).
struct Workspace {
    int* slabs = nullptr;
    int* ring_slabs = nullptr;                    // K-sliced ring kernel: sentinel-filled between launches (QS_SLAB_SENTINEL)
    unsigned* counters = nullptr;
    size_t slab_bytes = 0;
    int ncounters = 0;
    bool tried = false;
};
Workspace g_ws[16][QS_MAX_STREAM_SLOTS];   // [device][scratch slot] (common.h)

Workspace* get_workspace(hipStream_t stream) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return nullptr;
    Workspace& w = g_ws[dev][qs_scratch_slot(stream)];
    if (!w.tried) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(stream, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) {
            (void)hipGetLastError();
            return nullptr;                       // first use inside a capture: run un-split, allocate on a later eager call
        }
        w.tried = true;
        const size_t slab_bytes = 48u << 20;
        const int ncnt = 1 << 16;
        void *a = nullptr, *b = nullptr, *c = nullptr;
        if (hipMalloc(&a, slab_bytes) == hipSuccess && hipMalloc(&b, ncnt * sizeof(unsigned)) == hipSuccess &&
            hipMalloc(&c, slab_bytes) == hipSuccess && hipMemset(c, 0x80, slab_bytes) == hipSuccess &&
            hipMemset(b, 0, ncnt * sizeof(unsigned)) == hipSuccess && hipDeviceSynchronize() == hipSuccess) {
            w.slabs = reinterpret_cast<int*>(a);
            w.ring_slabs = reinterpret_cast<int*>(c);
            w.counters = reinterpret_cast<unsigned*>(b);
            w.slab_bytes = slab_bytes;
            w.ncounters = ncnt;
        } else {
            (void)hipGetLastError();
        }
    }
    return w.slabs ? &w : nullptr;
}
// K-sliced ring launches (gemm_w4a8_ring.hip, the seam) keep one int32 slab of mt x 4 KiB per (64-channel tile, token block, K
// slice) in `ring_slabs` and one arrival counter per (tile, token block); the last counter is the slot's error word, never a ticket
bool ring_workspace_fits(const Workspace& w, int N, int mt, int mblocks, int ksplit) {
    const size_t tiles = (size_t)(N / 64) * mblocks;
    return tiles < (size_t)w.ncounters && tiles * ksplit * mt * 4096 <= w.slab_bytes;
}
}  // namespace
// the error word of the GEMM hand-offs of a scratch slot: the LAST ticket counter (never used as a ticket: see ring_ws / launch_splitk)
unsigned* qs_gemm_error_word(int slot) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16 || slot < 0 || slot >= QS_MAX_STREAM_SLOTS) return nullptr;
    Workspace& w = g_ws[dev][slot];
    return w.slabs ? w.counters + (w.ncounters - 1) : nullptr;
}
bool qs_gemm_scratch_prealloc(hipStream_t stream) { return get_workspace(stream) != nullptr; }
int qs_gemm_reset_handoff() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return QS_OK;
    for (int slot = 0; slot < QS_MAX_STREAM_SLOTS; ++slot) {
        Workspace& w = g_ws[dev][slot];
        if (!w.slabs) continue;
        hipError_t e = hipMemset(w.ring_slabs, 0x80, w.slab_bytes);
        if (e == hipSuccess) e = hipMemset(w.counters, 0, (size_t)w.ncounters * sizeof(unsigned));
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) {
            qs_set_error("qs_device_reset (gemm): %s", hipGetErrorString(e));
            return (int)e;
        }
    }
    return QS_OK;
}
namespace {

template <int MT, int MODE, int OUTK, int NSTAGE>
int launch_splitk(const GemmArgs& a, int NW, int S, bool xcd_map) {
    auto kern = w4a8_gemm_splitk<MT, MODE, OUTK, NSTAGE>;
    size_t smem = NW > 1 ? (size_t)NW * MT * 16 * 64 * sizeof(int) : 16;
    // (not qs_reserve_lds: the reservation grows with the wave count of the launch)
    static size_t configured_dev[QS_MAX_DEVICES] = {};   // per instantiation and device
    size_t& configured = configured_dev[qs_device_slot()];
    if (smem > configured) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (e != hipSuccess) {
            qs_set_error("w4a8 gemm: cannot reserve %zu bytes of LDS: %s", smem, hipGetErrorString(e));
            return (int)e;
        }
        configured = smem;
    }
    dim3 grid(a.N / 64, (a.M + 16 * MT - 1) / (16 * MT), 1);
    int mblocks = 0;
    if (xcd_map && grid.y > 1 && grid.x % 8 == 0 && S == 1) {   // 1-D XCD-aware mapping (see kernel)
        mblocks = grid.y;
        grid.x *= grid.y;
        grid.y = 1;
    }
    int* slabs = nullptr;
    unsigned* counters = nullptr;
    if (S > 1) {
        Workspace* ws = get_workspace(a.stream);
        const size_t tiles = (size_t)grid.x * grid.y;
        const size_t need = tiles * S * (size_t)(MT * 4 * 64) * 16;
        if (ws && need <= ws->slab_bytes && tiles < (size_t)ws->ncounters) {     // (the last counter is the error word)
            slabs = ws->slabs;
            counters = ws->counters;
            grid.z = S;
        }
    }
    hipLaunchKernelGGL(kern, grid, dim3(NW * 64), smem, a.stream, a.A, a.W, a.zeros, a.scales8, a.wscales, a.ascales, a.wszs,
                       a.assums, a.out, slabs, counters, a.M, a.N, a.K, mblocks, g_epi_fma);
    return qs_launch_status("w4a8 gemm");
}

constexpr int QS_UNFUSED = 1 << 20;   // internal: the chosen kernel has no activation epilogue

int require_shape(int M, int N, int K) {
    const ShapeFault f = gemm_plan::check_shape(M, N, K);
    QS_REQUIRE(f != SHAPE_BAD, "w4a8 gemm: bad shape M=%d N=%d K=%d", M, N, K);
    QS_REQUIRE(f != SHAPE_N_NOT_64, "w4a8 gemm: N=%d must be a multiple of 64", N);
    QS_REQUIRE(f != SHAPE_K_NOT_128, "w4a8 gemm: K=%d must be a multiple of 128", K);
    return QS_OK;
}
// GEMM_INVALID: the planner reports the forced geometry that does not fit, the caller says so
int reject_plan(const GemmPlan& plan, int M, int N, int K) {
    qs_set_error("w4a8 gemm: forced ring geometry mt=%d wn=%d ksplit=%d does not fit M=%d N=%d K=%d", plan.p[0], plan.p[1],
                 plan.p[3], M, N, K);
    return QS_EINVAL;
}

// One GEMM: validate, plan (gemm_plan.h), launch.  MODE / OUTK as in gemm_w4a8.h; act: the silu * mul epilogue (outk 2) where a
// family has it, QS_UNFUSED where the plan is GEMM_NONE.
template <int MODE, int OUTK>
int dispatch(const GemmArgs& a, bool act = false) {
    const int outk = act ? 2 : OUTK;
    const int M = a.M, N = a.N, K = a.K;
    if (int rc = require_shape(M, N, K)) return rc;
    if (M == 0) return QS_OK;   // empty batch: nothing to do (zero-size tensors carry null pointers)
    QS_REQUIRE(a.A && a.W && a.out, "w4a8 gemm: null pointer");
    if (OUTK == 0) QS_REQUIRE(a.wscales && a.ascales, "w4a8 gemm: null scale pointer");
    if (MODE == 0 && OUTK == 0) QS_REQUIRE(a.wszs && a.assums, "w4a8 per-channel gemm: null w_szs / a_ssums");
    if (MODE == 1) QS_REQUIRE(a.zeros && a.scales8, "w4a8 per-group gemm: null zeros / scales_i8");
    const int variant = g_variant;
    GemmPlan plan = plan_w4a8(MODE, act, M, N, K, variant);
    if (plan.family == GEMM_INVALID) return reject_plan(plan, M, N, K);
    const int* p = plan.p;
    int* slabs = nullptr;
    unsigned* counters = nullptr;
    if (plan.family == GEMM_RING && p[3] > 1) {   // K slices meet in the workspace
        Workspace* ws = get_workspace(a.stream);
        if (ws && ring_workspace_fits(*ws, N, p[0], p[2], p[3])) {
            slabs = ws->ring_slabs;
            counters = ws->counters;
        } else {   // no workspace (e.g. first call inside a capture)
            QS_REQUIRE(variant < QS_GEMM_RING_GEOMETRY_BASE || variant >= QS_GEMM_RING_GEOMETRY_END,
                       "w4a8 gemm: no split-K workspace for the forced geometry");
            plan = ring_unsplit_plan(M, N, K);
        }
    }
    switch (plan.family) {
    case GEMM_WIDE: return qs_launch_gemm_wide(MODE, outk, a, g_tiled_order / 10);
    case GEMM_TILED: return qs_launch_gemm_tiled(MODE, outk, a, p[0]);
    case GEMM_RING: return qs_launch_gemm_ring(MODE, outk, p[0], p[1], a, p[2], p[3], slabs, counters);
    case GEMM_PAIR: return qs_launch_gemm_pair(MODE, OUTK, a);   // (OUTK: an `act` plan never reaches this family)
    case GEMM_SPLITK:
        switch (p[0]) {
        case 1: return launch_splitk<1, MODE, OUTK, 2>(a, p[1], p[2], p[3]);
        case 2: return launch_splitk<2, MODE, OUTK, 2>(a, p[1], p[2], p[3]);
        case 3: return launch_splitk<3, MODE, OUTK, 2>(a, p[1], p[2], p[3]);
        case 4: return launch_splitk<4, MODE, OUTK, 2>(a, p[1], p[2], p[3]);
        }
        qs_set_error("w4a8 gemm: unsupported split-K tile of %d m-tiles", p[0]);
        return QS_ENOSUP;
    default: return QS_UNFUSED;
    }
}

// the common fields of an entry's record; the entry names the rest
GemmArgs gemm_args(const int8_t* in_feats, const int8_t* kernel, void* out, int M, int N, int K, qs_stream_t stream) {
    GemmArgs a = {};
    a.A = in_feats, a.W = reinterpret_cast<const uint8_t*>(kernel), a.out = out;
    a.M = M, a.N = N, a.K = K, a.stream = reinterpret_cast<hipStream_t>(stream);
    return a;
}
const __half* half_ptr(const void* p) { return reinterpret_cast<const __half*>(p); }

}  // namespace

extern "C" void qs_set_gemm_variant(int variant) {
    // the sticky families keep their own word (include/qserve_amd.h qs_gemm_variant_code); every other code is the planner's
    if (variant >= QS_GEMM_TILED_DEBUG_BASE && variant < QS_GEMM_TILE_ORDER_BASE) g_tiled_dbg = variant - QS_GEMM_TILED_DEBUG_BASE;
    else if (variant >= QS_GEMM_TILE_ORDER_BASE && variant < QS_GEMM_ACT_FUSED)
        g_tiled_order = variant - QS_GEMM_TILE_ORDER_BASE, g_wide_order = (variant - QS_GEMM_TILE_ORDER_BASE) % 10;
    else if (variant >= QS_GEMM_WIDE_DEBUG_BASE && variant < QS_GEMM_WIDE_DEBUG_BASE + 100) g_wide_dbg = variant - QS_GEMM_WIDE_DEBUG_BASE;
    else if (variant == QS_GEMM_ACT_FUSED || variant == QS_GEMM_ACT_SPLIT) g_act_off = variant - QS_GEMM_ACT_FUSED;
    else if (variant >= QS_GEMM_RING_FLAGS_BASE && variant < QS_GEMM_RING_FLAGS_END) g_ring_flags = variant - QS_GEMM_RING_FLAGS_BASE;
    else g_variant = variant;
}

// Per-channel epilogue convention (include/qserve_amd.h): 0 = (acc*ws)*sa - wz*ss with every operation rounded separately
// (default), 1 = fmaf(acc*ws, sa, -(wz*ss)).  Process-wide, read at launch time by every W4A8 per-channel GEMM launch and by
// qs_add_residual_rms_norm_general_planes (which finishes such a GEMM).
qs_flag g_epi_fma = 0;
extern "C" int qs_set_gemm_epilogue(int convention) {
    QS_REQUIRE(convention == 0 || convention == 1, "qs_set_gemm_epilogue: convention %d not in {0, 1}", convention);
    g_epi_fma = convention;
    return QS_OK;
}
extern "C" int qs_get_gemm_epilogue(void) { return g_epi_fma; }

unsigned long long* g_gemm_clk = nullptr;
int g_gemm_clk_cap = 0;
extern "C" int qs_debug_gemm_clock_probe(void* buf, int workgroups) {
    QS_REQUIRE((buf == nullptr) == (workgroups == 0) && workgroups >= 0, "qs_debug_gemm_clock_probe: buffer and capacity come together");
    g_gemm_clk = reinterpret_cast<unsigned long long*>(buf);
    g_gemm_clk_cap = workgroups;
    return QS_OK;
}

extern "C" int qs_w4a8_gemm_plan(int per_group, int M, int N, int K, int* plan5) {
    QS_REQUIRE(plan5, "w4a8 gemm plan: null output");
    for (int i = 0; i < 5; ++i) plan5[i] = 0;
    if (int rc = require_shape(M, N, K)) return rc;
    if (M == 0) return QS_OK;
    const GemmPlan plan = plan_w4a8(per_group ? 1 : 0, false, M, N, K, g_variant);
    if (plan.family == GEMM_INVALID) return reject_plan(plan, M, N, K);
    plan5[0] = plan.family;
    for (int i = 0; i < 4; ++i) plan5[1 + i] = plan.p[i];
    return QS_OK;
}

extern "C" int qs_w4a8_per_chn_gemm(const int8_t* in_feats, const int8_t* kernel, const void* wscales,
                                    const void* ascales, const void* w_szs, const void* a_ssums, void* out_feats,
                                    int M, int N, int K, qs_stream_t stream) {
    GemmArgs a = gemm_args(in_feats, kernel, out_feats, M, N, K, stream);
    a.wscales = half_ptr(wscales), a.ascales = half_ptr(ascales), a.wszs = half_ptr(w_szs), a.assums = half_ptr(a_ssums);
    return dispatch<0, 0>(a);
}

extern "C" int qs_w4a8_per_group_gemm(const int8_t* in_feats, const int8_t* kernel, const int8_t* zeros,
                                      const int8_t* scales_i8, const void* wscales, const void* ascales,
                                      void* out_feats, int M, int N, int K, qs_stream_t stream) {
    GemmArgs a = gemm_args(in_feats, kernel, out_feats, M, N, K, stream);
    a.zeros = zeros, a.scales8 = scales_i8, a.wscales = half_ptr(wscales), a.ascales = half_ptr(ascales);
    return dispatch<1, 0>(a);
}

// gate_up GEMM + silu_and_mul in one launch where the kernel family has the epilogue, as two launches through `tmp`
// ([M, N] fp16) otherwise - bit-identical either way (the epilogue applies silu_and_mul's arithmetic to the fp16-rounded
// GEMM outputs)
qs_flag g_act_off = 0;   // qs_set_gemm_variant(3301 / 3300): always two launches / default (A/B, tests)
namespace {
template <int MODE>
int gate_up_silu(const GemmArgs& a, void* tmp) {   // a.out = out_act [M, N/2]
    QS_REQUIRE(a.N > 0 && a.N % 128 == 0, "w4a8 gate_up + silu: N=%d must stack two multiples of 64 channels", a.N);
    if (a.M == 0) return QS_OK;
    QS_REQUIRE(a.out, "w4a8 gate_up + silu: null output");
    int rc = g_act_off ? QS_UNFUSED : dispatch<MODE, 0>(a, true);
    if (rc != QS_UNFUSED) return rc;
    QS_REQUIRE(tmp, "w4a8 gate_up + silu: this shape needs the [M, N] fp16 scratch `tmp` (two launches)");
    GemmArgs plain = a;
    plain.out = tmp;
    rc = dispatch<MODE, 0>(plain);
    if (rc != QS_OK) return rc;
    return qs_silu_and_mul(a.out, tmp, a.M, a.N / 2, reinterpret_cast<qs_stream_t>(a.stream));
}
}  // namespace

extern "C" int qs_w4a8_per_chn_gemm_silu_mul(const int8_t* in_feats, const int8_t* kernel, const void* wscales,
                                             const void* ascales, const void* w_szs, const void* a_ssums,
                                             void* out_act, void* tmp, int M, int N, int K, qs_stream_t stream) {
    GemmArgs a = gemm_args(in_feats, kernel, out_act, M, N, K, stream);
    a.wscales = half_ptr(wscales), a.ascales = half_ptr(ascales), a.wszs = half_ptr(w_szs), a.assums = half_ptr(a_ssums);
    return gate_up_silu<0>(a, tmp);
}

extern "C" int qs_w4a8_per_group_gemm_silu_mul(const int8_t* in_feats, const int8_t* kernel, const int8_t* zeros,
                                               const int8_t* scales_i8, const void* wscales, const void* ascales,
                                               void* out_act, void* tmp, int M, int N, int K, qs_stream_t stream) {
    GemmArgs a = gemm_args(in_feats, kernel, out_act, M, N, K, stream);
    a.zeros = zeros, a.scales8 = scales_i8, a.wscales = half_ptr(wscales), a.ascales = half_ptr(ascales);
    return gate_up_silu<1>(a, tmp);
}

// ---- K-slice planes -----------------------------------------------------------------------------------------------------------
// The row-parallel GEMMs of a layer (o, down) are followed by a ROW kernel that reads their whole output anyway (residual add
// + norm + quant).  In this form the GEMM leaves its K slices as int32 planes [k_slices][M][N] - no cross-workgroup seam, no
// epilogue - and qs_add_residual_rms_norm_general_planes sums the planes and applies the GEMM's epilogue arithmetic itself:
// the kernel boundary that is there anyway is the hand-off (in-launch it costs a 2.4-3 us round trip under load, see
// gemm_w4a8_ring.hip).  Geometry: gemm_plan.h planes_plan.
namespace {
template <int MODE>
int gemm_planes(const GemmArgs& a) {   // a.out = planes
    QS_REQUIRE(a.A && a.W && a.out && (MODE == 0 || (a.zeros && a.scales8)), "w4a8 gemm (planes): null pointer");
    const GemmPlan g = planes_plan(MODE, a.M, a.N, a.K, g_variant);
    if (g.family != GEMM_RING) {
        qs_set_error("w4a8 gemm (planes): no ring geometry for M=%d N=%d K=%d (ask qs_w4a8_gemm_planes_plan first)", a.M, a.N, a.K);
        return QS_ENOSUP;
    }
    return qs_launch_gemm_ring(MODE, 3, g.p[0], g.p[1], a, g.p[2], g.p[3], nullptr, nullptr);
}
}  // namespace

extern "C" int qs_w4a8_gemm_planes_plan(int per_group, int M, int N, int K, int* plan4) {
    QS_REQUIRE(plan4, "w4a8 gemm planes plan: null output");
    const GemmPlan g = planes_plan(per_group ? 1 : 0, M, N, K, g_variant);   // GEMM_NONE (all zero: k_slices == 0): not available, run the pair
    plan4[0] = g.p[3], plan4[1] = g.p[0], plan4[2] = g.p[1], plan4[3] = g.p[2];
    return QS_OK;
}
extern "C" int qs_w4a8_per_chn_gemm_planes(const int8_t* in_feats, const int8_t* kernel, int32_t* planes, int M, int N, int K,
                                           qs_stream_t stream) {
    return gemm_planes<0>(gemm_args(in_feats, kernel, planes, M, N, K, stream));
}
extern "C" int qs_w4a8_per_group_gemm_planes(const int8_t* in_feats, const int8_t* kernel, const int8_t* zeros,
                                             const int8_t* scales_i8, int32_t* planes, int M, int N, int K, qs_stream_t stream) {
    GemmArgs a = gemm_args(in_feats, kernel, planes, M, N, K, stream);
    a.zeros = zeros, a.scales8 = scales_i8;
    return gemm_planes<1>(a);
}

extern "C" int qs_w4a8_per_chn_gemm_acc(const int8_t* in_feats, const int8_t* kernel, int32_t* acc_out, int M, int N,
                                        int K, qs_stream_t stream) {
    return dispatch<0, 1>(gemm_args(in_feats, kernel, acc_out, M, N, K, stream));
}

extern "C" int qs_w4a8_per_group_gemm_acc(const int8_t* in_feats, const int8_t* kernel, const int8_t* zeros,
                                          const int8_t* scales_i8, int32_t* acc_out, int M, int N, int K,
                                          qs_stream_t stream) {
    GemmArgs a = gemm_args(in_feats, kernel, acc_out, M, N, K, stream);
    a.zeros = zeros, a.scales8 = scales_i8;
    return dispatch<1, 1>(a);
}
