// attn_plan.h -- which attention kernel serves a call, with what geometry and how many KV splits: every planner of the decode
// (attention.hip, attention_mfma*.hip) and the append families (append_attention*.hip, append_tree.hip, append_shared.hip), stated
// ONCE.  Plain C++17: no HIP, no device access, no global state, no error reporting - a plan is a function of its arguments alone
// (the capacity of the split-KV workspace is one of them), so the whole table can be printed and pinned on a machine without a GPU
// (tests/host/attn_plan_table.cpp, tests/test_attn_plan_table_cpu.py).  The launchers run what these functions return;
// qs_attention_plan, qs_append_attention_plan, qs_append_attention_split_plan and qs_append_shared_plan report it.
//
// Every constant below is measured or named as a starting value: a change must come with new measurements and a re-recorded
// tests/golden/attn_plan_table.json.
#pragma once
#include <cstddef>

namespace attn_plan {

// ---- the geometry the kernels are built for (append_walk.h and attention.hip assert that they agree) ----------------
constexpr int PAGE = 64;             // tokens per KV page = keys per tile of the append kernels
constexpr int DH = 128;              // head_dim
constexpr int APPEND_WAVES = 4;      // waves per workgroup of the append kernels, 32 rows each
constexpr int APPEND_ROWS = 32 * APPEND_WAVES;
constexpr int DECODE_WAVES_KV4 = 8;  // waves per workgroup of the matrix-core decode kernels (attention_mfma.hip, attention_mfma8.hip)
constexpr int DECODE_WAVES_KV8 = 4;
constexpr int DECODE_WAVES_VALU = 4; // ... and of the VALU kernel (attention.hip)
constexpr int DECODE_LDS_PAGES = 192;
// Split-KV partial records of the append family (append_attention_split.hip has the layout): one block per (workgroup of the
// un-split grid, split, wave)
constexpr int REC_FLOATS = 32 * (DH + 2);          // O^T [32 chunks][32 rows][4], m[32], l[32]
constexpr int MAX_SPLITS = 64;

// ---- the split-KV workspace: bytes of ONE split's records, and the cut of a wanted split count to what the workspace holds ----
// decode kernels: a record of O[128], m, l per (sequence, KV head) workgroup and query head of its group
inline size_t decode_split_bytes(int blocks, int G) { return (size_t)blocks * G * (DH + 2) * sizeof(float); }
// append family (linear and tree): a block of REC_FLOATS per wave of each of `wgs` un-split workgroups
inline size_t append_split_bytes(size_t wgs) { return wgs * APPEND_WAVES * REC_FLOATS * sizeof(float); }
// the effective count for a wanted one: at most max_splits and what `capacity` bytes hold; 1 (= run un-split) where fewer than two
// sets fit.  (The decode launchers have no cap of their own: NO_SPLIT_CAP.)
constexpr int NO_SPLIT_CAP = 0x7fffffff;
inline int fit_splits(int wanted, size_t per_split_bytes, size_t capacity, int max_splits) {
    int splits = wanted > max_splits ? max_splits : wanted;
    if (per_split_bytes * splits > capacity) splits = (int)(capacity / per_split_bytes);
    return splits > 1 ? splits : 1;
}

// ---- decode attention (qs_single_query_attention, qs_attention_plan) ---------------------------------------------------------
// Split-KV factor of the matrix-core decode kernels (KV4: attention_mfma.hip, KV8: attention_mfma8.hip): the number of workgroups a
// (sequence, KV head) pair's page range is cut into.  Cost model fitted to a sweep on the MI355X (profiles/round5_split_sweep*.txt:
// 1 .. 48 sequences x 8 KV heads, 1 030 .. 7 700 tokens, 1 .. 32 splits; mean regret 0.7 %, worst 10 %, against the forced best;
// the round-2 rule "aim at >= 512 workgroups" it replaces: 8 % / 39 %):
//   time(n) = rounds * F + max(rounds * pages / n * t_cu,  blocks * pages * t_hbm) + merge(n)
// rounds = ceil(blocks * n / 256): workgroups land on the 256 CUs round-robin and a CU streams at its own request budget whatever
// the number of resident workgroups, so 320 workgroups take as long as 512; F = a workgroup's head + tail; t_cu = one CU's time
// per page (64 tokens of K and V), t_hbm = the chip's; merge = the second launch (boundary + n partials per head).
// ns / ps units, integer arithmetic (the plan is part of the ABI: tests/test_dispatch_plan.py pins it).
inline int qs_attn_choose_splits(int blocks, int pages, int kv8, int fused_quant) {
    if (blocks >= 512 || pages < 4) return 1;
    const long F = kv8 ? 5000 : 4000, t_cu = kv8 ? 450 : 340, t_hbm_ps = kv8 ? 2540 : 1330;
    long best = -1;
    int best_n = 1;
    // (n <= 8: within this kernel's range - page tables of <= 192 entries, 12 288 tokens; longer tables go to the VALU kernels -
    //  more splits do not pay: 1 / 2 / 4 sequences at 8 191 and 12 200 tokens, forced 4 / 8 / 12 / 16 / 24 splits against this
    //  choice, KV4 and KV8: the choice is the best or within 1 % of it everywhere except one sequence of 12 200 tokens over an INT8
    //  cache, where 12 splits measure 20.4 against 21.7 us - profiles/round6_split_long.txt.  ADVICE r05 extrapolated the cost
    //  formula to 512 pages, which this function is never asked about.)
    for (int n = 1; n <= 8; ++n) {
        if (n > 1 && pages / n < 2) break;
        const long rounds = ((long)blocks * n + 255) / 256;
        const long per_cu = rounds * pages * t_cu / n, chip = (long)blocks * pages * t_hbm_ps / 1000;
        // (fused_quant: qs_single_query_attention_quant - only the un-split launch can finish the row itself; a split one is
        // followed by the quantiser as a launch of its own, 3.2 us + boundary)
        const long cost = rounds * F + (per_cu > chip ? per_cu : chip) + (n > 1 ? 2500 + 300 * n + (fused_quant ? 3500 : 0) : 0);
        if (best < 0 || cost < best) best = cost, best_n = n;
    }
    return best_n;
}
// The decode attention kernel choice, from the problem and the selection hook `variant` alone (qs_attention_plan reports it,
// single_query_attention launches it; the codes of `variant` are listed at g_attn_variant, attention.hip).  fused_quant: the
// attention + quant entry asks.
// family 1 = matrix-core KV4, 2 = matrix-core KV8, 3 = VALU kernel, 0 = rejected: num_heads / num_kv_heads not in 1..8 (the caller
// words the error); nsplit = KV splits (workgroups per sequence and KV head: the launchers cut it to what their workspace holds);
// waves per workgroup; kflags = KV4 kernel switches (variants 5 and 7); exp_flags = KV4 ablation builds of the G = 4 kernel
// (200 + bits, QS_TIMING builds)
struct AttnPlan {
    int family, nsplit, waves, kflags, exp_flags;
};
inline AttnPlan plan_attention(int batch, int H, int Hkv, int max_blocks, int timestep, bool int4, bool fused_quant, int variant) {
    const int G = H / Hkv;
    if (G < 1 || G > 8) return {0, 0, 0, 0, 0};
    // the matrix-core kernel caches a sequence's page addresses in LDS (192 pages = 12288 tokens per sequence); longer
    // page tables take the VALU kernel
    if (variant == 1 || max_blocks > DECODE_LDS_PAGES) return {3, 1, DECODE_WAVES_VALU, 0, 0};
    int force_split = variant >= 100 ? variant - 100 : 0, exp_flags = 0;
    if (int4 && force_split >= 100) {
        exp_flags = force_split - 100;
        force_split = 0;
    }
    const int blocks = Hkv * batch;
    const int pages_max = (timestep + PAGE - 1) / PAGE;
    const int nsplit = force_split > 0 ? force_split : qs_attn_choose_splits(blocks, pages_max, int4 ? 0 : 1, int4 && fused_quant && H * DH <= 4096);
    if (int4) return {1, nsplit, DECODE_WAVES_KV4, variant == 5 ? 2 : variant == 7 ? 1024 : 0, exp_flags};
    return {2, nsplit, DECODE_WAVES_KV8, 0, 0};
}

// ---- append attention: geometry of a launch - the ONE statement of it (the plan entries and the launchers all ask here) --------
struct AppendPlan {
    int tile_tokens, q_tiles, waves;
};
inline AppendPlan plan_append(int max_seqlen_q, int num_heads, int num_kv_heads) {
    const int G = num_heads / num_kv_heads;
    AppendPlan p;
    p.waves = APPEND_WAVES;
    p.tile_tokens = APPEND_ROWS / G; // rows = (token, head-in-group): every head of the group rides on the same staged tiles
    p.q_tiles = (max_seqlen_q + p.tile_tokens - 1) / p.tile_tokens;
    return p;
}

// ---- split-KV append attention (qs_append_attention_split_plan; the tree entry asks the same planner) --------------------------
// "Fill the CUs once" (the decode chooser's form): the un-split grid has base = batch * Hkv * q_tiles workgroups and the
// chip holds FILL of them at a time (256 CUs x two 64 KiB workgroups); below that, split until the chip is full, but never below
// MIN_PAGES pages per split (a split pays its own Q load, pipeline fill, 65 KiB of partial records and its share of the merge) and
// never for a past of fewer than 128 tokens.
// Fitted to scripts/bench_append_split.py -> profiles/append_split.txt (MI355X, Llama-3-8B heads):
//   FILL = 512       B = 8, past 4096, n = 4 (base 64): 4 splits 44 us, 7 splits (what the workspace holds of 512 / 64 = 8) 40 us -
//                    filling both workgroup slots of every CU still pays; no correction to the starting form.
//   MIN_PAGES = 8    B = 1, past 8192, n = 8: 16 splits (8 pages each) 33.6 us KV4 / 35.1 us KV8, 32 splits (4 pages each) 34.0 /
//                    37.8 us - below 8 pages per split the merge and the per-split set-up cost what the shorter chain saves.
//                    At short pasts it is too high (B = 1, n = 8, past 1024: 2 splits 25.9 us, 8 splits 18.0 us; past 2048: 4 splits
//                    26.8 us, 8 splits 21.6 us - still ahead of un-split, 37.0 / 65.2 us): the regret is in the profile and DESIGN 10.
constexpr int FILL = 512;
constexpr int MIN_PAGES = 8;
inline int plan_splits(int batch, int q_tiles, int num_kv_heads, int max_past, size_t capacity) {
    const long base = (long)batch * num_kv_heads * q_tiles;
    if (base <= 0 || base >= FILL || max_past < 2 * PAGE) return 1;
    const int pages = (max_past + PAGE - 1) / PAGE;
    long s = FILL / base;
    if (s > pages / MIN_PAGES) s = pages / MIN_PAGES;
    const long cap = (long)(capacity / append_split_bytes((size_t)base));
    if (s > cap) s = cap;
    if (s > MAX_SPLITS) s = MAX_SPLITS;
    return s < 1 ? 1 : (int)s;
}

// ---- shared-prefix append attention (qs_append_shared_plan) ------------------------------------------------------------------
// The split planner's form ("fill the CUs once", the chip holds FILL = 512 workgroups) with the two roles'
// base grids counted TOGETHER - they share the launch.  Their chains differ by an order of magnitude (B = 64, prefix 1 024, own past
// 64: 64 prefix workgroups of 16 pages next to 512 suffix workgroups of 2 tiles), so a workgroup counts with its chain length: the
// launch holds  tiles = base_prefix * prefix pages + base_suffix * (suffix pages + 1)  tile walks, a slot of the chip gets tiles / FILL
// of them, and a role with `pages` pages is cut into  pages / (tiles / FILL)  ranges.  With one role this is the split planner's
// FILL / base; counting the workgroups unweighted would give FILL / 576 = 0 -> P = 1 at the shape above, one serial walk of 16 pages.
// Then: never below a minimum of pages per split and role, at most 64 splits, and cut to what the workspace holds (the suffix role
// keeps one set of records; the prefix role gives way first, down to P = 0 = "do not share").
//   MIN_PAGES (suffix)     the split planner's constant (the suffix role IS its workgroup).
//   MIN_PAGES_PREFIX = 2   the prefix role's own; the STARTING value - the sweep of scripts/bench_append_shared.py that is to fix it (lowest
//                          worst regret over its table) has not been run on an MI355X yet: not measured.
constexpr int MIN_PAGES_PREFIX = 2;

struct SharedPlan {
    int tq, q_tiles, waves, S, gq_tiles, P, rw_suffix, rw_prefix;
    size_t bytes;
};
// the waves of a workgroup that can own a row (append_shared.hip: the records of the others are not laid out)
inline int rec_waves(int tq, int max_tokens, int G) {
    const int rows = (max_tokens < tq ? max_tokens : tq) * G;
    const int w = (rows + 31) / 32;
    return w < 1 ? 1 : w > APPEND_WAVES ? APPEND_WAVES : w;
}
constexpr size_t REC_BYTES = REC_FLOATS * sizeof(float);
// bytes of one set (one split) of a role's records
inline size_t set_bytes(long wgs, int rw) { return (size_t)wgs * rw * REC_BYTES; }
// cut (P, S) to the workspace: S first gives way down to 1, then P down to 0
inline void fit_workspace(int& P, int& S, size_t per_p, size_t per_s, size_t cap) {
    if (per_s > cap) {      // not even one set of suffix records
        P = 0;
        return;
    }
    if (P > (int)((cap - per_s) / per_p)) P = (int)((cap - per_s) / per_p);
    if (S > (int)((cap - (size_t)P * per_p) / per_s)) S = (int)((cap - (size_t)P * per_p) / per_s);
}
inline int splits_for(int pages, long tiles, int min_pages) {
    long s = (long)pages * FILL / tiles;
    if (s > pages / min_pages) s = pages / min_pages;
    if (s > MAX_SPLITS) s = MAX_SPLITS;
    return s < 1 ? 1 : (int)s;
}
// force_p / force_s: 0 = choose, >= 1 = that count (cut to 64 and the workspace), force_p = -1 = do not share
inline SharedPlan plan_shared(int batch, int max_seqlen_q, int num_groups, int max_group_tokens, int max_prefix, int max_suffix_past,
                              int num_heads, int num_kv_heads, int force_p, int force_s, size_t capacity) {
    const int G = num_heads / num_kv_heads;
    const AppendPlan ap = plan_append(max_seqlen_q, num_heads, num_kv_heads);
    SharedPlan p = {};
    p.tq = ap.tile_tokens, p.q_tiles = ap.q_tiles, p.waves = ap.waves;
    p.gq_tiles = (max_group_tokens + p.tq - 1) / p.tq;
    p.rw_suffix = rec_waves(p.tq, max_seqlen_q, G), p.rw_prefix = rec_waves(p.tq, max_group_tokens, G);
    const long base_p = (long)num_groups * p.gq_tiles * num_kv_heads, base_s = (long)batch * p.q_tiles * num_kv_heads;
    const int pages_p = max_prefix / PAGE, pages_s = (max_suffix_past + PAGE - 1) / PAGE;
    const long tiles = base_p * pages_p + base_s * (pages_s + 1);
    const bool share = force_p >= 0 && (force_p > 0 || (num_groups < batch && max_prefix >= PAGE));
    if (share) {
        p.P = force_p > 0 ? (force_p > MAX_SPLITS ? MAX_SPLITS : force_p) : splits_for(pages_p, tiles, MIN_PAGES_PREFIX);
        p.S = force_s > 0 ? (force_s > MAX_SPLITS ? MAX_SPLITS : force_s) : splits_for(pages_s, tiles, MIN_PAGES);
        fit_workspace(p.P, p.S, set_bytes(base_p, p.rw_prefix), set_bytes(base_s, p.rw_suffix), capacity);
        p.bytes = (size_t)p.P * set_bytes(base_p, p.rw_prefix) + (size_t)p.S * set_bytes(base_s, p.rw_suffix);
    }
    if (p.P == 0) p.S = 0, p.bytes = 0, p.rw_prefix = 0, p.rw_suffix = APPEND_WAVES;      // the split entry's launch: the caller asks its planner
    return p;
}

}  // namespace attn_plan
