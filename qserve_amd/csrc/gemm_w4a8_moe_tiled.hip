// gemm_w4a8_moe_tiled.hip -- compute-bound grouped W4A8 GEMM for mixture-of-experts prompts: the second form behind
// qs_w4a8_per_*_moe_gemm (contract: include/qserve_amd.h; the weight-streaming form and the entries are gemm_w4a8_moe.hip).
//
//   out[p, :] = W[e] x[row_src[p], :]   for every sorted position p < P, e = the expert whose range of expert_offsets holds p.
//
// The streaming kernel streams an expert's weights once per 64 sorted rows; with thousands of rows per expert (a prompt) that is the
// weights tens of times over.  This kernel is a tile in the manner of gemm_w4a8_tiled.hip, grouped:
//   * workgroup = 8 wave64 computes (expert, 128 sorted rows, 256 channels); wave (wm, wn) owns 64 rows x one 64-channel unit: 4
//     m-tiles x 4 row classes of v_mfma_i32_16x16x64_i8, 64 accumulator VGPRs.  128 rows, not 256: expert ranges are ragged and the
//     last block of every expert is partly empty.
//   * both operands reach LDS by LDS-DMA in stages of 64 k: 8 KiB of packed weights (+ 512 B of level-2 scales / zeros) per stage in
//     a 6-deep ring, the activations as stage PAIRS of 16 KiB in a 3-deep ring, so that every DMA instruction fetches whole 128-byte
//     lines of 8 rows (gemm_w4a8_tiled.hip's header has the measurement behind that).  101 376 B of LDS, one workgroup per CU.
//   * the gather costs nothing: the DMA takes a per-lane source address, and a lane's is row_src[p] * x_stride + its place in the
//     row, computed once per tile.  Rows are never expanded or copied.
//   * LDS images are bank-conflict free by permuting the SOURCE addresses (the DMA writes lane-linear): the dense tile's pair image
//     for the activations and its [tile][chunk][k32 ^ tile][c] image for the weights.
//   * one raw s_barrier per stage, counted s_waitcnt vmcnt keeps the later stages in flight across it; inside a stage a wave runs 16
//     MFMAs and between them reads the next stage's operands, unpacks its weight nibbles (per-group: level-2 dequant in registers,
//     bit-faithful) and issues its share of the DMA for the stage five ahead.
//   * block -> expert: the streaming kernel's search with R = 128 - lane e holds expert e, a wave prefix sum of the block counts,
//     ballot + readlane name the expert.  The grid is the host-known bound of moe_plan.h; surplus workgroups leave at once; rows past
//     the expert's range are computed on a clamped row and not stored.  No cross-workgroup wait of any kind.
//   * launch order: a 1-D grid walked in super-tiles of 16 row blocks x 16 channel tiles, row blocks fastest: the 256 workgroups in
//     flight share 16 weight tiles - of one expert where the expert has 2 048 rows - and 16 blocks of activation rows.
//   * the epilogue's scales are requested before the k loop (they belong to the SOURCE row: a dependent load behind row_src) and the
//     fp16 tile is staged through LDS so that every store instruction writes whole 128-byte rows.
// Index hygiene as in the streaming kernel: offsets clamped into [0, P], a range that runs backwards is empty, row_src clamped into
// [0, x_rows - 1].  Per-lane offsets are 32-bit; the expert's base goes into the scalar base pointer (moe_plan::tiled_serves).
#include "gemm_w4a8_moe.h"
#include "moe_plan.h"

namespace {

constexpr int NS = 6;                      // weight ring depth (stages of 64 k); the activation ring holds NS / 2 stage pairs
constexpr int MT = 4;                      // m-tiles of a wave
constexpr int BM = moe_plan::TILED_ROWS;
constexpr int BN = moe_plan::TILED_CHANNELS;
constexpr int WSTAGE = BN * 32;            // packed weight bytes per stage = 8 KiB
constexpr int APAIR = BM * 128;            // activation bytes per stage pair = 16 KiB
constexpr int NA2 = APAIR / 8192;          // all-thread DMA instructions per activation pair
constexpr int LDS_BYTES = NS * (BM * 64 + WSTAGE + 512);
typedef __attribute__((address_space(3))) void* lptr_t;

template <int N>
__device__ __forceinline__ void wait_vm() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// counted wait with a run-time count (pipeline fill and drain only; the steady state uses a constant)
__device__ __forceinline__ void wait_vm_dyn(int n) {
    switch (n) {
#define QS_W(N) case N: wait_vm<N>(); break
        QS_W(1); QS_W(2); QS_W(3); QS_W(4); QS_W(5); QS_W(6); QS_W(7); QS_W(8);
#undef QS_W
    default: wait_vm<0>(); break;
    }
}
__device__ __forceinline__ void raw_barrier() {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// MODE 0 = per-channel, 1 = per-group(128)
template <int MODE>
__global__ __launch_bounds__(512, 1) void w4a8_moe_gemm_tiled(
    const int8_t* __restrict__ X, long long x_stride, int x_rows, const int* __restrict__ row_src, const int* __restrict__ offsets,
    const uint8_t* __restrict__ Wall, const int8_t* __restrict__ zeros_all, const int8_t* __restrict__ scales8_all,
    const __half* __restrict__ wscales_all, const __half* __restrict__ ascales, const __half* __restrict__ wszs_all,
    const __half* __restrict__ assums, _Float16* __restrict__ out, long long out_stride, int P, int E, int N, int K, int nrb,
    int epi_fma) {
    constexpr int NW = 1 + (MODE == 1 ? 1 : 0);       // DMA instructions per stage for the weights (+ per-group meta)
    static_assert(NA2 + NW <= MT && NS % 2 == 0, "pipeline slots");
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint8_t* const a_ring = smem;                     // [NS/2][APAIR]  pair image (gemm_w4a8_tiled.hip)
    uint8_t* const w_ring = smem + (NS / 2) * APAIR;  // [NS][unit 4][tile 2][e 4][k32^tile 2][c 8][16 B]
    uint8_t* const m_ring = w_ring + NS * WSTAGE;     // [NS][512]: 256 scales | 256 zeros (storage order)

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;
    const int li = lane & 15, g = lane >> 4;
    const int tsel = li >> 3, c = li & 7;

    // ---- (row block, channel tile) of this workgroup: super-tiles of 16 x 16, row blocks fastest (only the last band of channel
    // tiles and the last group of row blocks are narrower, and they come last in their direction)
    const int nbn = N / BN;
    int bm, bn;
    {
        const int id = blockIdx.x;
        const int band = id / (nrb * 16), in_band = id - band * (nrb * 16);
        const int wid = nbn - band * 16 < 16 ? nbn - band * 16 : 16;
        const int grp = in_band / (16 * wid), in_grp = in_band - grp * (16 * wid);
        const int hgt = nrb - grp * 16 < 16 ? nrb - grp * 16 : 16;
        bm = grp * 16 + in_grp % hgt;
        bn = band * 16 + in_grp / hgt;
    }

    // ---- (expert, first row) of row block bm, from the offsets: every wave does the same search (all 64 lanes active)
    int lo = 0, hi = 0;
    if (lane < E) {
        lo = offsets[lane], hi = offsets[lane + 1];
        lo = lo < 0 ? 0 : lo > P ? P : lo;
        hi = hi < 0 ? 0 : hi > P ? P : hi;
    }
    const int nblk = hi > lo ? (hi - lo + BM - 1) / BM : 0;
    int incl = nblk;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    const int first = incl - nblk;
    const unsigned long long owner = __ballot(nblk > 0 && bm >= first && bm < incl);
    if (owner == 0) return;                                        // surplus block (workgroup-uniform, before any barrier)
    const int e = __builtin_amdgcn_readfirstlane(__ffsll((long long)owner) - 1);
    const int row0 = __builtin_amdgcn_readlane(lo, e) + (bm - __builtin_amdgcn_readlane(first, e)) * BM;
    const int row_end = __builtin_amdgcn_readlane(hi, e);          // row0 < row_end <= P
    const int n0 = bn * BN;

    const int KT = K >> 5;
    const int nh = K >> 6;                            // stages (even: K % 128 == 0; >= 4)
    auto source_row = [&](int p) {                    // sorted position -> source row, both clamped into what exists
        p = p < row_end ? p : row_end - 1;
        int s = row_src ? row_src[p] : p;
        return s < 0 ? 0 : s >= x_rows ? x_rows - 1 : s;
    };

    // the SOURCE rows of this lane's four output rows (the epilogue's scales belong to them), read with the DMA's rows below
    int esrc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) esrc[mt] = source_row(row0 + wm * (16 * MT) + 16 * mt + li);

    // ---- DMA sources: per-lane 32-bit byte offsets; the k advance and the expert go into the scalar base ------------------------
    // (inline asm rather than __builtin_amdgcn_global_load_lds: the compiler books the builtin as a FLAT access and from then on
    //  degrades every counted LDS wait in the loop to lgkmcnt(0))
    // activations: instruction i of a wave copies tile rows (i * 8 + wave) * 8 .. + 7 as one 1 KiB piece of the pair image: half h
    // of row 2a + b sits at 64-byte position 4a + 2 (h ^ (a & 1)) + b, chunk c of row j at 16-byte position c ^ ((-(j >> 2)) & 3)
    auto aswz = [&](int j) { return (0 - j) & 3; };
    u32 a_off[NA2];
    {
        const int a_r0 = wave * 8 + 2 * (lane >> 4) + ((lane >> 2) & 1);
        const u32 a_c = ((((lane >> 3) & 1) ^ ((lane >> 4) & 1)) * 64) + (((lane & 3) ^ aswz((a_r0 >> 2) & 3)) * 16);
#pragma unroll
        for (int i = 0; i < NA2; ++i)
            a_off[i] = (u32)source_row(row0 + a_r0 + 64 * i) * (u32)x_stride + a_c;   // x_rows * x_stride < 2^32 (the launcher's caller)
    }
    // weights: wave w copies tile row w (32 channels) of the tile's eight; per-group meta: dword `lane` of the tile's 64
    const u32 w_off = ((u32)wave * (u32)KT + (((lane >> 3) & 1) ^ (wave & 1))) * 512u + (lane & 7) * 64 + (lane >> 4) * 16;
    const u32 m_off = lane * 4;
    const uint8_t* const w_base = Wall + (size_t)e * N * (size_t)(K >> 1) + (size_t)(n0 / 32) * KT * 512;
    const int8_t* const m_base = MODE == 1 ? ((wave & 1) ? zeros_all : scales8_all) + (size_t)e * (K >> 7) * N + n0 : nullptr;
    const u32 lds0 = (u32)(size_t)(lptr_t)smem;

    auto dma16 = [&](u32 voff, const void* sbase, u32 lds_addr) {
        asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(sbase), "s"(lds_addr)
                     : "memory");
    };
    auto dma4 = [&](u32 voff, const void* sbase, u32 lds_addr) {
        asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %0, %1" ::"v"(voff), "s"(sbase), "s"(lds_addr)
                     : "memory");
    };
    auto issue_a = [&](int pr, int pslot, int i) {                 // instruction i of activation pair pr (stages 2 pr, 2 pr + 1)
        dma16(a_off[i], X + (size_t)pr * 128, lds0 + pslot * APAIR + (i * 8 + wave) * 1024);
    };
    auto issue_w = [&](int u, int slot, int i) {                   // i = 0: weights of stage u, 1: its per-group meta
        if (i == 0) dma16(w_off, w_base + (size_t)u * 1024, lds0 + (NS / 2) * APAIR + slot * WSTAGE + wave * 1024);
        else dma4(m_off, m_base + (size_t)(u >> 1) * N, lds0 + (NS / 2) * APAIR + NS * WSTAGE + slot * 512 + (wave & 1) * 256);
    };
    // Issue order of a wave (vmcnt retires in order): W(0), then for q = 0, 1, ...: A(q), W(2q+1), W(2q+2).  The fill issues
    // W(0..4), A(0), A(1); stage u issues W(u+5) and, when u is even, A(u/2 + 2) before it.  Stage v reads its own and ALREADY
    // stage v+1's operands, so before stage v the wave needs everything up to W(v+1) (v even; A(v/2) precedes it) or up to
    // A((v+1)/2) (v odd; W(v+1) precedes it) complete; whatever was issued later may stay in flight: 3 NW + NA2 instructions in
    // the steady state, `allowed(v)` at the ends of K.
    auto allowed = [&](int v) {
        const int nw = v + 5 < nh ? v + 5 : nh, na = 2 + ((v + 1) >> 1) < (nh >> 1) ? 2 + ((v + 1) >> 1) : (nh >> 1);
        const int q = v >> 1;
        const int need = (v & 1) ? NW + (q + 1) * (NA2 + 2 * NW) + NA2 : 2 * NW + q * (NA2 + 2 * NW) + NA2;
        return NW * nw + NA2 * na - need;          // <= 0 at the end of K: everything has to be there
    };

    // ---- LDS operand readers ----------------------------------------------------------------------------------------------------
    const int w_rd = wn * 2048 + tsel * 1024 + (((g >> 1) ^ tsel)) * 128 + c * 16 + (g & 1) * 8;   // + chunk * 256
    const int m_rd = wn * 64 + (tsel * 8 + c) * 4;
    const int a_rd0 = (2 * wm * MT + (li >> 3)) * 1024 + (4 * ((li & 7) >> 1) + 2 * ((li >> 1) & 1) + (li & 1)) * 64 +
                      ((g ^ aswz(li >> 2)) * 16);                                                  // half 0; + mt * 2048
    auto read_b = [&](int pslot, int half, int mt) -> v4i {
        return *reinterpret_cast<const v4i*>(a_ring + pslot * APAIR + (a_rd0 ^ (half * 128)) + mt * 2048);
    };
    struct Raw {
        v2u r[4];
        u32 sdw, zdw;
    };
    // per-group: four separate address registers keep these 8-byte reads from being merged into ds_read2_b64, which this image is
    // not laid out for (gemm_w4a8_tiled.hip has the A/B: per-group gains, per-channel loses)
    int w_rd_e[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        w_rd_e[q] = w_rd + q * 256;
        if (MODE == 1) asm volatile("" : "+v"(w_rd_e[q]));
    }
    auto read_w = [&](int slot) -> Raw {
        Raw q;
#pragma unroll
        for (int j = 0; j < 4; ++j) q.r[j] = *reinterpret_cast<const v2u*>(w_ring + slot * WSTAGE + w_rd_e[j]);
        q.sdw = 0;
        q.zdw = 0;
        if (MODE == 1) {
            q.sdw = *reinterpret_cast<const u32*>(m_ring + slot * 512 + m_rd);
            q.zdw = *reinterpret_cast<const u32*>(m_ring + slot * 512 + 256 + m_rd);
        }
        return q;
    };
    auto build = [&](const Raw& q, int cl) -> v4i {
        u32 s = 0, zb = 0;
        if (MODE == 1) {
            s = (q.sdw >> (8 * cl)) & 0xFFu;
            zb = ((q.zdw >> (8 * cl)) & 0xFFu) * 0x01010101u;
        }
        v4i a;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const u32 raw = (cl & 1) ? q.r[j].y : q.r[j].x;
            a[j] = (int)((cl & 2) ? unpack_hi<MODE>(raw, s, zb) : unpack_lo<MODE>(raw, s, zb));
        }
        return a;
    };

    v4i acc[MT][4];
    v4i a0[4], a1[4], bq[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int cl = 0; cl < 4; ++cl) acc[mt][cl] = (v4i){0, 0, 0, 0};

    // ---- pipeline fill: weights of stages 0 .. NS - 2 and two activation pairs in flight (K >= 256: both pairs exist)
#pragma unroll
    for (int i = 0; i < NW; ++i) issue_w(0, 0, i);
#pragma unroll
    for (int q = 0; q < 2; ++q) {
#pragma unroll
        for (int i = 0; i < NA2; ++i) issue_a(q, q, i);
#pragma unroll
        for (int t = 1; t <= 2; ++t)
            if (2 * q + t < nh) {
#pragma unroll
                for (int i = 0; i < NW; ++i) issue_w(2 * q + t, 2 * q + t, i);
            }
    }

    // ---- epilogue operands, requested behind the fill and read after the k loop: the scales of this wave's channels and of its
    // SOURCE rows.  (They are younger than the fill, so the counted waits of the first stages over-wait by these loads, never under.)
    const int ncol0 = n0 + 64 * wn + 32 * (g >> 1) + 4 * (g & 1);
    h4 ws4[4], wz4[4];
    _Float16 sa_h[MT], ss_h[MT];
#pragma unroll
    for (int cl = 0; cl < 4; ++cl) {
        ws4[cl] = *reinterpret_cast<const h4*>(reinterpret_cast<const _Float16*>(wscales_all) + (size_t)e * N + ncol0 + 8 * cl);
        if (MODE == 0) wz4[cl] = *reinterpret_cast<const h4*>(reinterpret_cast<const _Float16*>(wszs_all) + (size_t)e * N + ncol0 + 8 * cl);
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        sa_h[mt] = reinterpret_cast<const _Float16*>(ascales)[esrc[mt]];
        if (MODE == 0) ss_h[mt] = reinterpret_cast<const _Float16*>(assums)[esrc[mt]];
    }

    // One stage = 16 MFMAs of this wave. `ac` holds the unpacked weight operands of stage u, `an` receives those of stage u + 1;
    // bq[mt] is m-tile mt's activation operand: read for stage u + 1 as soon as stage u has used it.  PAR = u & 1.
    auto stage = [&](auto par_c, auto pref_static, bool pref_a, bool pref_w, int u, int slot, v4i(&ac)[4], v4i(&an)[4]) {
        constexpr int PAR = decltype(par_c)::value;
        constexpr bool st = decltype(pref_static)::value;
        const int slot_n = slot + 1 == NS ? 0 : slot + 1;
        const int slot_d = slot == 0 ? NS - 1 : slot - 1;          // (u + NS - 1) % NS
        const int ps = slot >> 1, ps_n = slot_n >> 1;              // activation pair slots of stage u / u + 1
        const int ps_d = ps == 0 ? NS / 2 - 1 : ps - 1;            // (u / 2 + 2) % (NS / 2)
        Raw qn;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const v4i b_use = bq[mt];
            bq[mt] = read_b(ps_n, PAR ^ 1, mt);
            if (mt == 0) qn = read_w(slot_n);
            if (PAR == 0 && mt < NA2) {
                if (st || pref_a) issue_a((u >> 1) + 2, ps_d, mt);
            } else if (mt - (PAR == 0 ? NA2 : 0) < NW) {
                if (st || pref_w) issue_w(u + NS - 1, slot_d, mt - (PAR == 0 ? NA2 : 0));
            }
            if (mt >= 2) {
                an[2 * (mt - 2)] = build(qn, 2 * (mt - 2));
                an[2 * (mt - 2) + 1] = build(qn, 2 * (mt - 2) + 1);
            }
#pragma unroll
            for (int cl = 0; cl < 4; ++cl) acc[mt][cl] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ac[cl], b_use, acc[mt][cl], 0, 0, 0);
            // (per-channel: the read / DMA / unpack order is pinned between the MFMA groups; with the VALU-heavy per-group dequant
            //  the compiler's own interleaving measured faster in the dense tile)
            if (MODE == 0) __builtin_amdgcn_sched_barrier(0);
        }
    };
    // barrier before stage u: stage u + 1 has landed (this wave's pieces by the counted wait; the barrier extends that to every
    // wave's) while later stages stay in flight, and every wave is done reading stage u - 1, whose slot is refilled next
    using c0 = std::integral_constant<int, 0>;
    using c1 = std::integral_constant<int, 1>;
    wait_vm_dyn(allowed(0));
    raw_barrier();
    {
        const Raw q0 = read_w(0);
#pragma unroll
        for (int t = 0; t < MT; ++t) bq[t] = read_b(0, 0, t);
#pragma unroll
        for (int cl = 0; cl < 4; ++cl) a0[cl] = build(q0, cl);
    }
    int slot = 0, u = 0;
    for (; u + NS < nh; u += 2) {                      // steady state: both stages of the pair prefetch, no branches
        if (u) {                                       // (u = 0: the fill's wait and barrier)
            wait_vm<3 * NW + NA2>();
            raw_barrier();
        }
        stage(c0{}, std::true_type{}, true, true, u, slot, a0, a1);
        slot = slot + 1 == NS ? 0 : slot + 1;
        wait_vm<3 * NW + NA2>();
        raw_barrier();
        stage(c1{}, std::true_type{}, true, true, u + 1, slot, a1, a0);
        slot = slot + 1 == NS ? 0 : slot + 1;
    }
    for (; u < nh; u += 2) {                           // drain: request what is left of K, wait for more each stage
        if (u) {
            wait_vm_dyn(allowed(u));
            raw_barrier();
        }
        stage(c0{}, std::false_type{}, u + 4 < nh, u + NS - 1 < nh, u, slot, a0, a1);
        slot = slot + 1 == NS ? 0 : slot + 1;
        wait_vm_dyn(allowed(u + 1));
        raw_barrier();
        stage(c1{}, std::false_type{}, false, u + NS < nh, u + 1, slot, a1, a0);
        slot = slot + 1 == NS ? 0 : slot + 1;
    }

    // ---- epilogue: the dense entries' (common.h), scales of the expert's channels and of the SOURCE row -------------------------
    raw_barrier();                                     // the rings are dead: every wave left the k loop, every DMA has landed
    // The fp16 tile of this wave goes through LDS, 16 rows x 64 channels at a time, so that every store instruction writes whole
    // 128-byte rows (the accumulator layout would scatter 8-byte pieces over 32 lines per instruction).  The staging rows are written
    // and read by the same wave: an LDS wait, no barrier.
    constexpr int RS = 144;                            // staged row stride (bytes): 128 + 16 keeps 16-byte alignment
    uint8_t* const st = a_ring + wave * (16 * RS);
    _Float16* const orow = out + n0 + wn * 64 + (lane & 7) * 8;
    // the per-channel convention (qs_set_gemm_epilogue) is a wave-uniform branch around two copies of the loop, not a select per element
    auto store_tile = [&](auto fma_c) {
        constexpr int FMA = decltype(fma_c)::value;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const float sa = (float)sa_h[mt];
            const float ss = MODE == 0 ? (float)ss_h[mt] : 0.f;
#pragma unroll
            for (int cl = 0; cl < 4; ++cl) {
                const v4i s = acc[mt][cl];
                h4 o;
                if (MODE == 0) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        // the fp32 value is made opaque before it is narrowed: left to itself the compiler fuses the FMA convention's
                        // fmaf and the conversion into v_fma_mixlo_f16, which rounds ONCE to fp16 - not the dense entries' two roundings
                        float v = epi_per_chn(s[r], (float)ws4[cl][r], sa, (float)wz4[cl][r], ss, FMA);
                        asm("" : "+v"(v));
                        o[r] = (_Float16)v;
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) o[r] = (_Float16)epi_per_group(s[r], (float)ws4[cl][r], sa);
                }
                *reinterpret_cast<h4*>(st + li * RS + (32 * (g >> 1) + 8 * cl + 4 * (g & 1)) * 2) = o;
            }
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int r = i * 8 + (lane >> 3);
                const int m = row0 + wm * (16 * MT) + 16 * mt + r;
                const v4u v = *reinterpret_cast<const v4u*>(st + r * RS + (lane & 7) * 16);
                if (m < row_end) *reinterpret_cast<v4u*>(orow + (size_t)m * (size_t)out_stride) = v;
            }
        }
    };
    if (MODE == 0 && epi_fma) store_tile(std::integral_constant<int, 1>());
    else store_tile(std::integral_constant<int, 0>());
}

template <int MODE>
int launch_moe_tiled(const MoeArgs& a) {
    auto kern = w4a8_moe_gemm_tiled<MODE>;
    static bool lds_reserved[QS_MAX_DEVICES] = {};   // per instantiation (= kernel) and device
    if (const hipError_t e = qs_reserve_lds({reinterpret_cast<const void*>(kern)}, LDS_BYTES, lds_reserved); e != hipSuccess) {
        qs_set_error("w4a8 moe gemm (tiled): cannot reserve %d bytes of LDS: %s", LDS_BYTES, hipGetErrorString(e));
        return (int)e;
    }
    const moe_plan::MoeTiledPlan pl = moe_plan::plan_moe_tiled(a.P, a.E, a.N, a.K);
    hipLaunchKernelGGL(kern, dim3((unsigned)pl.rblocks * (unsigned)pl.ntiles), dim3(512), LDS_BYTES, a.stream, a.x, (long long)a.x_stride,
                       a.x_rows, a.row_src, a.offsets, reinterpret_cast<const uint8_t*>(a.qweight), a.zeros, a.scales8,
                       reinterpret_cast<const __half*>(a.wscales), reinterpret_cast<const __half*>(a.ascales),
                       reinterpret_cast<const __half*>(a.wszs), reinterpret_cast<const __half*>(a.assums),
                       reinterpret_cast<_Float16*>(a.out), (long long)a.out_stride, a.P, a.E, a.N, a.K, pl.rblocks, (int)g_epi_fma);
    return qs_launch_status("w4a8 moe gemm (tiled)");
}

}  // namespace

int qs_launch_moe_tiled(int mode, const MoeArgs& a) { return mode == 0 ? launch_moe_tiled<0>(a) : launch_moe_tiled<1>(a); }
