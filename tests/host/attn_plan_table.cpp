// attn_plan_table.cpp -- prints the attention planners' whole decision table (qserve_amd/csrc/attn_plan.h), one line per grid point:
//
//   D variant fused_quant int4 H Hkv max_blocks batch timestep : family nsplit waves kflags exp_flags      plan_attention
//   A n H Hkv : tile_tokens q_tiles waves                                                                  plan_append
//   S batch n H Hkv max_past : splits                                                                      plan_splits
//   P force_p force_s batch groups n max_group_tokens H Hkv max_suffix_past max_prefix :
//         tile_tokens q_tiles waves S group_q_tiles P rec_waves_suffix rec_waves_prefix bytes unshared_splits    plan_shared
//         (unshared_splits: what plan_splits gives the whole past where P = 0 - the split entry's launch; 0 elsewhere)
//   F max_splits wanted per_split_bytes : splits                                                           fit_splits
//
// over the capacity of the library's split-KV workspace (32 MiB).  A host program: it includes the planner header and nothing else
// of the library.  tests/test_attn_plan_table_cpu.py compiles it, compares its output with tests/golden/attn_plan_table.json
// (recorded before the planners moved into the header), ties the rows it can to the built library's plan entries and asserts that
// the grid reaches every cut of the planners.  Built with -fsanitize=address,undefined it also checks the planners' integer
// arithmetic over the whole grid.
#include <climits>
#include <cstdio>
#include <initializer_list>

#include "../../qserve_amd/csrc/attn_plan.h"

using namespace attn_plan;

static const size_t CAP = (size_t)32 << 20;
static const int HEADS[][2] = {{32, 8}, {8, 2}, {4, 4}, {8, 1}, {6, 2}, {12, 4}, {5, 1}, {7, 1}, {16, 8}, {28, 4}, {64, 8}};   // tests/test_append_cpu.py's
static const int FEW_HEADS[][2] = {{32, 8}, {8, 2}, {64, 8}};
static const int DECODE_HEADS[][2] = {{32, 8}, {8, 2}, {64, 8}, {72, 8}};      // (72 / 8: nine query heads per KV head - rejected)
static const int SHARED_HEADS[][2] = {{32, 8}, {8, 2}, {4, 4}, {8, 1}, {7, 1}, {16, 8}, {64, 8}};                           // tests/test_append_shared_cpu.py's

static void shared_row(int fp, int fs, int batch, int groups, int n, int mgt, int H, int Hkv, int ms, int mp) {
    const SharedPlan p = plan_shared(batch, n, groups, mgt, mp, ms, H, Hkv, fp, fs, CAP);
    const long whole = (long)mp + ms;
    const int unshared = p.P == 0 ? plan_splits(batch, p.q_tiles, Hkv, whole > INT_MAX ? INT_MAX : (int)whole, CAP) : 0;
    std::printf("P %d %d %d %d %d %d %d %d %d %d : %d %d %d %d %d %d %d %d %zu %d\n", fp, fs, batch, groups, n, mgt, H, Hkv, ms, mp, p.tq, p.q_tiles,
                p.waves, p.S, p.gq_tiles, p.P, p.rw_suffix, p.rw_prefix, p.bytes, unshared);
}

int main() {
    // ---- decode: every variant family, both cache types, the fused-quant term on both sides of H * 128 <= 4096 (32 / 64 heads), a group
    // size out of range (72 / 8), page tables on both sides of 192, timesteps from 2 pages to 12 288 tokens
    for (int variant : {0, 1, 3, 5, 7, 101, 102, 103, 108, 112, 116, 201, 232})
        for (int fq = 0; fq < 2; ++fq)
            for (int int4 = 1; int4 >= 0; --int4)
                for (const auto& h : DECODE_HEADS)
                    for (int mb : {64, 192, 193})
                        for (int batch : {1, 2, 4, 8, 16, 32, 48, 64, 128})
                            for (int ts : {100, 255, 256, 257, 511, 1030, 2048, 4096, 7700, 8191, 12288}) {
                                const AttnPlan p = plan_attention(batch, h[0], h[1], mb, ts, int4 != 0, fq != 0, variant);
                                std::printf("D %d %d %d %d %d %d %d %d : %d %d %d %d %d\n", variant, fq, int4, h[0], h[1], mb, batch, ts, p.family,
                                            p.nsplit, p.waves, p.kflags, p.exp_flags);
                            }
    // ---- append geometry
    for (int n : {0, 1, 4, 8, 33, 130, 512})
        for (const auto& h : HEADS) {
            const AppendPlan p = plan_append(n, h[0], h[1]);
            std::printf("A %d %d %d : %d %d %d\n", n, h[0], h[1], p.tile_tokens, p.q_tiles, p.waves);
        }
    // ---- split planner: the sweep of tests/test_append_split_cpu.py
    for (int batch : {0, 1, 4, 64})
        for (int n : {0, 1, 8, 33, 512})
            for (const auto& h : HEADS)
                for (int mp : {0, 63, 64, 127, 128, 1024, 8192, 32768, 131072})
                    std::printf("S %d %d %d %d %d : %d\n", batch, n, h[0], h[1], mp,
                                plan_splits(batch, plan_append(n, h[0], h[1]).q_tiles, h[1], mp, CAP));
    // ---- shared planner, unforced: the sweep of tests/test_append_shared_cpu.py (empty launches have no plan: the entries return first)
    static const int BG[][2] = {{1, 1}, {4, 1}, {4, 2}, {4, 4}, {64, 1}, {64, 8}, {64, 64}};
    for (const auto& bg : BG)
        for (int n : {1, 4, 33, 512})
            for (const auto& h : SHARED_HEADS)
                for (int ms : {0, 64, 1024, 8192})
                    for (int mp : {0, 63, 64, 128, 1024, 8192, 131072}) shared_row(0, 0, bg[0], bg[1], n, n * (bg[0] / bg[1]), h[0], h[1], ms, mp);
    // ---- shared planner, forced counts; max_group_tokens = 2048 makes one set of PREFIX records larger than what the suffix set leaves
    static const int FBG[][2] = {{4, 1}, {4, 4}, {64, 1}, {64, 8}};
    static const int HINTS[][2] = {{1024, 0}, {64, 1024}, {8192, 8192}, {131072, 131072}};   // max_suffix_past, max_prefix
    for (int fp : {-1, 0, 1, 3, 64, 100})
        for (int fs : {0, 1, 5, 100})
            for (const auto& bg : FBG)
                for (int n : {1, 4, 33, 300})
                    for (int mgt : {n * (bg[0] / bg[1]), 2048})
                        for (const auto& h : FEW_HEADS)
                            for (const auto& sp : HINTS) shared_row(fp, fs, bg[0], bg[1], n, mgt, h[0], h[1], sp[0], sp[1]);
    // ---- the cut of a wanted split count: the append family's cap of 64, the decode launchers' none
    for (int max_splits : {MAX_SPLITS, NO_SPLIT_CAP})
        for (int wanted : {1, 2, 3, 8, 63, 64, 65, 100, 1000})
            for (size_t bytes : {(size_t)0, (size_t)1, decode_split_bytes(8, 4), append_split_bytes(1), append_split_bytes(8), (size_t)1 << 20, CAP / 3,
                                 CAP / 2, CAP / 2 + 1, CAP, CAP + 1, append_split_bytes(1024)})
                std::printf("F %d %d %zu : %d\n", max_splits, wanted, bytes, fit_splits(wanted, bytes, CAP, max_splits));
    return 0;
}
