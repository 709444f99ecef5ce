// gemm_plan_table.cpp -- prints the W4A8 GEMM planner's whole decision table: one line per (variant, per_group, act, M, N, K)
//
//     variant per_group act M N K <plan> <fallback> <planes>
//
//   <plan>      X forced geometry that does not fit | N no kernel with the activation epilogue | P pair | Tm tiled | Wm wide |
//               Rmt,wn,mblocks,ksplit ring | Smt,nw,s,xcd split-K
//   <fallback>  Umt,wn,mblocks: what a K-sliced ring plan runs as without a workspace; - for every other plan
//   <planes>    ks,mt,wn,mblocks of the K-slice planes form; 0 where it is not available
//
// A host program: it includes the planner header and nothing else of the library.  tests/test_gemm_plan_table_cpu.py compiles
// it, compares its output with tests/golden/gemm_plan_table.json (recorded before the three ring searches were merged) and
// ties the rows it can to the built library's plan entries.  Built with -fsanitize=address,undefined it also checks the cost
// model's integer products over the whole grid.
#include <cstdio>
#include <vector>

#include "../../qserve_amd/csrc/gemm_plan.h"

using namespace gemm_plan;

static const int MS[] = {1, 8, 16, 17, 32, 33, 48, 64, 65, 96, 128, 129, 191, 192, 255, 256, 257, 383, 384, 512, 1024, 1025, 2048, 4096, 65536};

static const int NK[][2] = {
    // Llama-3-8B, its tensor-parallel shards, other models' down / gate_up (tests/test_dispatch_plan.py)
    {6144, 4096}, {4096, 4096}, {28672, 4096}, {4096, 14336}, {3072, 4096}, {1536, 4096}, {768, 4096}, {4096, 2048},
    {4096, 1024}, {14336, 4096}, {3584, 4096}, {4096, 7168}, {4096, 1792}, {49152, 4096},
    {49152, 8192}, {57344, 8192}, {8192, 8192}, {8192, 24576}, {4096, 11008}, {5120, 13824},
    // tests/test_gemm_gpu.py: small, short K, N % 128 != 0, N % 256 != 0
    {4096, 512}, {64, 128}, {128, 256}, {768, 512}, {65536, 1024},
    {4160, 4096}, {4224, 4096},
    // K / ks > 32768 for two slices only / for two and four; M * K >= 2^32 from M = 65536 / 32768 on; N * K / 2 >= 2^32;
    // K >= 2^24
    {4096, 131072}, {1024, 262144}, {4096, 65536}, {65536, 131072}, {256, 16777216},
};

int main() {
    std::vector<int> variants = {QS_GEMM_DEFAULT,
                                 QS_GEMM_PAIR_OFF, QS_GEMM_PAIR_FORCED, QS_GEMM_TILED_OFF, QS_GEMM_TILED_256, QS_GEMM_TILED_128,
                                 QS_GEMM_WIDE_256, QS_GEMM_RING_OFF, QS_GEMM_RING_NO_KSLICES, QS_GEMM_RING_NO_GROUP_TERM,
                                 QS_GEMM_RING_NO_DOWN_OVERRIDE, QS_GEMM_RING_NO_MT8};
    for (int code : {0, 18, 124, 222, 414, 937, 914, 99})   // 100 * mtile_override + 10 * S + NW, in and out of range
        variants.push_back(QS_GEMM_SPLITK_BASE + code);
    for (int base : {QS_GEMM_RING_GEOMETRY_BASE, QS_GEMM_PLANES_GEOMETRY_BASE})
        for (int ks : {1, 2, 4})
            for (const RingGeo& g : RING_GEO) variants.push_back(base + 100 * (ks - 1) + 10 * g.mt + g.wn);
    // forced geometries that do not exist (<0,0>, <1,2>, <8,1>, <4,3>, <8,4>, <9,9>) and three K slices
    for (int code : {0, 12, 81, 43, 84, 242, 399}) variants.push_back(QS_GEMM_RING_GEOMETRY_BASE + code);
    for (int code : {9, 199, 242}) variants.push_back(QS_GEMM_PLANES_GEOMETRY_BASE + code);

    for (int variant : variants)
        for (int pg = 0; pg < 2; ++pg)
            for (int act = 0; act < 2; ++act)
                for (const auto& nk : NK)
                    for (int M : MS) {
                        const int N = nk[0], K = nk[1];
                        if (check_shape(M, N, K) != SHAPE_OK) return 1;
                        std::printf("%d %d %d %d %d %d ", variant, pg, act, M, N, K);
                        const GemmPlan p = plan_w4a8(pg, act != 0, M, N, K, variant);
                        switch (p.family) {
                        case GEMM_INVALID: std::printf("X"); break;
                        case GEMM_NONE: std::printf("N"); break;
                        case GEMM_PAIR: std::printf("P"); break;
                        case GEMM_TILED: std::printf("T%d", p.p[0]); break;
                        case GEMM_WIDE: std::printf("W%d", p.p[0]); break;
                        case GEMM_RING: std::printf("R%d,%d,%d,%d", p.p[0], p.p[1], p.p[2], p.p[3]); break;
                        case GEMM_SPLITK: std::printf("S%d,%d,%d,%d", p.p[0], p.p[1], p.p[2], p.p[3]); break;
                        default: return 2;
                        }
                        if (p.family == GEMM_RING && p.p[3] > 1) {
                            const GemmPlan u = ring_unsplit_plan(M, N, K);
                            std::printf(" U%d,%d,%d", u.p[0], u.p[1], u.p[2]);
                        } else {
                            std::printf(" -");
                        }
                        const GemmPlan q = planes_plan(pg, M, N, K, variant);
                        if (q.family == GEMM_RING) std::printf(" %d,%d,%d,%d\n", q.p[3], q.p[0], q.p[1], q.p[2]);
                        else std::printf(" 0\n");
                    }
    return 0;
}
