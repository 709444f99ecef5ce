// lora_plan.h -- which form of the LoRA row update serves a call, and the grid of the grouped one.  Plain C++17 next to moe_plan.h:
// no HIP, no device access, no global state - a function of (T, rows_per_seq, slots) alone, so it can be asked on a machine without a
// GPU (qs_lora_rows_form, qs_lora_rows_grouped_tiles).  Both forms compute the same bits (lora_grouped.hip): the choice is cost only.
#pragma once

namespace lora_plan {

constexpr int TILE = 16;                  // rows of a tile, of either form
constexpr int GROUPED_MAX_SLOTS = 64;     // the grouped kernels keep one LDS counter per slot and pick the adapter with one ballot word

// Tiles the grouped form launches: adapter a with c_a > 0 rows needs ceil(c_a / 16) tiles, and at most min(slots, S) adapters have
// rows, S = T / rows_per_seq sequences.  That is the row_blocks argument of moe_plan.h with R = 16 and E = min(slots, S): the sum is
// at most ceil(T / 16) + min(slots, S) - 1 for EVERY id assignment, so the host never reads one.  Workgroups past the last real tile
// leave at once.
inline int grouped_tiles(int T, int rows_per_seq, int slots) {
    if (T <= 0 || rows_per_seq <= 0 || slots <= 0) return 0;
    const int S = T / rows_per_seq;
    return (T + TILE - 1) / TILE + (slots < S ? slots : S) - 1;
}

// Output column slices (of 512) a grouped expand workgroup walks: every workgroup repeats the id scan, so with many tiles a workgroup
// keeps its tile and its staged t for several slices.  `ysplit` workgroups share a tile's slices round-robin; enough of them to put
// about eight workgroups on each of the 256 CUs, no more.
inline int grouped_expand_ysplit(int tiles, int nslices) {
    if (tiles <= 0 || nslices <= 0) return 0;
    const int want = (2048 + tiles - 1) / tiles;
    return want < nslices ? want : nslices;
}

// What the grouped form serves at all: tiles that one sequence cannot fill (rows_per_seq < 16; from 16 on the rows form's tiles are
// full already), slots within the LDS counters, and at most GROUPED_MAX_SEQS sequences - every workgroup scans all S ids.
//
// GROUPED_MAX_SEQS is the largest S of the measured sweep 64, 256, 1024, 4096, 16384 (rows_per_seq = 1, r = 16, 8 adapters) at which
// the grouped form still beat the rows form by more than the sweep's run-to-run spread at both the qkv (4096 -> 6144) and the gate_up
// (4096 -> 28672) shape of Llama-3-8B (profiles/lora_grouped.txt, "S sweep"): grouped / rows = 0.71 / 0.46 at S = 256, 0.36 / 0.29 at
// 1024, 0.25 / 0.22 at 4096 and 0.25 / 0.21 at 16384, spread 0.03 at the most - the redundant scan never caught up inside the sweep,
// so the constant is the sweep's end, not a crossover; nothing beyond it was measured.
//
// GROUPED_MIN_SEQS is the small end of the same sweep: at S = 64 the grouped form LOSES at qkv (15.1 against 10.0 us, 1.51) and wins at
// gate_up by 0.91 only; at 64 x 12 rows it loses at all four linears (1.2 - 1.7), and the captured bs = 64 step pays +2 181 us for
// eight adapters against +1 859 us.  With a dozen tiles the call is a chain of dependent latencies, and finding the tile adds two
// barriers and a second walk over the ids in front of the first load of x.  The planner therefore keeps the rows form below 256
// sequences, the first S of the sweep where the grouped form wins at both shapes; below that the form stays reachable by name.
constexpr int GROUPED_MAX_SEQS = 16384;
constexpr int GROUPED_MIN_SEQS = 256;
inline const char* grouped_refusal(int T, int rows_per_seq, int slots) {
    if (rows_per_seq >= TILE) return "rows_per_seq >= 16: one sequence fills a tile, the rows form serves it";
    if (slots < 1 || slots > GROUPED_MAX_SLOTS) return "slots outside 1 .. 64 (one LDS counter and one ballot bit per slot)";
    if (rows_per_seq >= 1 && T / rows_per_seq > GROUPED_MAX_SEQS) return "more sequences than GROUPED_MAX_SEQS (every workgroup scans all ids)";
    return nullptr;
}

enum LoraForm { LORA_ROWS = 0, LORA_GROUPED = 1 };
inline LoraForm lora_form(int T, int rows_per_seq, int slots) {
    if (T <= 0 || rows_per_seq <= 0 || grouped_refusal(T, rows_per_seq, slots)) return LORA_ROWS;
    return T / rows_per_seq >= GROUPED_MIN_SEQS ? LORA_GROUPED : LORA_ROWS;
}

}  // namespace lora_plan
