// lora_plan.h -- which form of the LoRA row update serves a call, and the grids of the grouped and the prompt one.  Plain C++17 next
// to moe_plan.h: no HIP, no device access, no global state - a function of (T, rows_per_seq, slots) alone, so it can be asked on a
// machine without a GPU (qs_lora_rows_form, qs_lora_rows_grouped_tiles).  All three forms compute the same bits (lora_rows.hip,
// lora_prompt.hip): the choice is cost only.
#pragma once

namespace lora_plan {

constexpr int TILE = 16;                  // rows of a tile of the rows and the grouped form
constexpr int PROMPT_TILE = 64;           // rows of a tile of the prompt form: one 16-row MFMA block for each of the four waves
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

// ---- the prompt form (lora_prompt.hip): a tile is up to 64 consecutive rows of one sequence
inline int prompt_tiles(int T, int rows_per_seq) {
    if (T <= 0 || rows_per_seq <= 0) return 0;
    return T / rows_per_seq * ((rows_per_seq + PROMPT_TILE - 1) / PROMPT_TILE);
}

// K slices (of 512) a prompt shrink workgroup walks one after the other: slices run .. run + prompt_run - 1 of workgroup y = run /
// prompt_run, the last run short.  A wave keeps its rows' x and its accumulators for the whole run, so a long run is cheap; but the
// grid has to cover the 256 CUs several times (about four workgroups each, PROMPT_SHRINK_WGS; a workgroup is one wave per SIMD), so
// with few tiles the runs are short - one slice at the least - and with many they are long.  Every slice belongs to exactly one run.
constexpr int PROMPT_SHRINK_WGS = 1024;
inline int prompt_run(int tiles, int kslices) {
    if (tiles <= 0 || kslices <= 0) return 0;
    int runs = (PROMPT_SHRINK_WGS + tiles - 1) / tiles;
    if (runs > kslices) runs = kslices;
    return (kslices + runs - 1) / runs;
}

// Output column slices (of 512) a prompt expand workgroup walks, as grouped_expand_ysplit: a workgroup stages its tile's t once - a
// read of every K-slice plane of 64 rows - and keeps it for the slices blockIdx.y, blockIdx.y + ysplit, ...; about four workgroups for
// each of the 256 CUs.
inline int prompt_expand_ysplit(int tiles, int nslices) {
    if (tiles <= 0 || nslices <= 0) return 0;
    const int want = (1024 + tiles - 1) / tiles;
    return want < nslices ? want : nslices;
}

// What the prompt form serves at all: a sequence that fills one 16-row block of a tile.  Below that the other two forms serve the
// call.  No slot limit: the tile's adapter is one read of seq_adapter.
inline const char* prompt_refusal(int T, int rows_per_seq, int slots) {
    (void)T;
    (void)slots;
    if (rows_per_seq < TILE) return "rows_per_seq < 16: a sequence does not fill one wave's block, the rows and the grouped form serve it";
    return nullptr;
}

// Where the planner takes the prompt form.  The measured sweep (profiles/lora_prompt.txt, section 1: rows_per_seq 16, 32, 64, 128, 256,
// 1 024 at T = 4 096 and 16 384, r = 16, 8 adapters, both forms captured, in alternation, medians of three) has prompt / rows at the
// qkv (4096 -> 6144) / gate_up (4096 -> 28672) shape: rows_per_seq = 16 0.91 / 0.82 at T = 4 096 and 0.86 / 0.70 at 16 384; 32 0.94 /
// 0.77 and 0.84 / 0.66; 64 0.83 / 0.74 and 0.76 / 0.72; 256 0.82 / 0.75 and 0.76 / 0.72; o and down 0.68 - 0.90; the spread inside the
// run is 0.01 at the most but for the lines at rows_per_seq = 16 (0.04 - 0.06), and an earlier run of the same script had the same
// lines within 0.07 of these (gate_up at 16 384 rows from 64 rows per sequence on: 0.65 there).  The form won at EVERY point of the
// sweep by more than the spread, so both limits are ends of it, not crossovers:
//   PROMPT_MIN_ROWS_PER_SEQ  rows_per_seq = 16 would have won too (above), but the planner's answer "rows" for (4096, 16, 8) is pinned
//                            by tests/test_lora_grouped_cpu.py, so the limit is 17; 17 .. 31 lie between two measured wins.
//   PROMPT_MIN_ROWS          4 096, the smaller T of the sweep; nothing below it was measured (a 64-node tree at bs = 64 is 4 096 rows).
//   PROMPT_MAX_PLANNED_RANK  the planner cannot see r through (T, rows_per_seq, slots); `planned_for_rank` is asked behind it.  At r = 64
//                            the prompt form LOSES, 1.28 / 1.28 of the rows form at qkv / gate_up (section 2): its expand holds all r
//                            values of B for two columns and runs one wave per SIMD there.  r = 32 was not measured.  So a planned
//                            "prompt" becomes "rows" above r = 16, the measured rank; the form stays reachable by name at every rank.
constexpr int PROMPT_MIN_ROWS_PER_SEQ = 17;
constexpr int PROMPT_MIN_ROWS = 4096;
constexpr int PROMPT_MAX_PLANNED_RANK = 16;

enum LoraForm { LORA_ROWS = 0, LORA_GROUPED = 1, LORA_PROMPT = 2 };
inline LoraForm lora_form(int T, int rows_per_seq, int slots) {
    if (T <= 0 || rows_per_seq <= 0) return LORA_ROWS;
    if (!prompt_refusal(T, rows_per_seq, slots) && rows_per_seq >= PROMPT_MIN_ROWS_PER_SEQ && T >= PROMPT_MIN_ROWS) return LORA_PROMPT;
    if (grouped_refusal(T, rows_per_seq, slots)) return LORA_ROWS;
    return T / rows_per_seq >= GROUPED_MIN_SEQS ? LORA_GROUPED : LORA_ROWS;
}

// The planner's form `form` for a call of rank r (PROMPT_MAX_PLANNED_RANK has the measurement).
inline LoraForm planned_for_rank(LoraForm form, int r) { return form == LORA_PROMPT && r > PROMPT_MAX_PLANNED_RANK ? LORA_ROWS : form; }

}  // namespace lora_plan
