// score_plan.h -- the geometry of qs_score_rows (score_rows.hip): the tile, how the vocabulary is cut into splits, the order in which the
// grid walks (row tile, split) pairs and the workspace.  Plain C++17 next to moe_plan.h / lora_plan.h: no device access, no global state
// - a plan is a function of (rows, V, K, forced splits) alone, so it is tested on a machine without a GPU (qs_score_rows_plan,
// qs_score_rows_grid_position).  grid_position is the one function the kernel itself calls, hence its host / device mark.
//
// A workgroup owns TILE_ROWS rows and a contiguous range of vocabulary tiles of TILE_VOCAB columns; it walks K in stages of STAGE_K
// through a ring of DEPTH stages in LDS.  The vocabulary's ceil(V / TILE_VOCAB) tiles are cut into `splits` ranges of tiles_per_split
// tiles (the last one may be shorter, none is empty); a row has one partial record per split, merged in ascending split order.
#pragma once

#if defined(__HIPCC__)
#define QS_SCORE_HD __host__ __device__
#else
#define QS_SCORE_HD
#endif

namespace score_plan {

constexpr int TILE_ROWS = 128;        // rows of a workgroup's tile
constexpr int TILE_VOCAB = 256;       // vocabulary columns of one logit tile
constexpr int STAGE_K = 64;           // k per pipeline stage
constexpr int DEPTH = 3;              // stages in the LDS ring: 3 x (16 + 32) KiB = 144 KiB of the CU's 160
constexpr int RECORD_BYTES = 16;      // {max, sum, target logit, arg-max index} per (row, split)
constexpr int MAX_SPLITS = 64;        // what the merge reads per row, one thread walking them in order
constexpr int BAND_ROWS = 8;          // row tiles of a grid band (below)
// MODEL figures, not measurements (DESIGN.md "Scoring prompts" says what they rest on):
constexpr int TARGET_WORKGROUPS = 512;   // two rounds of the chip's 256 CUs at one workgroup per CU
constexpr int MIN_TILES_PER_SPLIT = 2;   // a split shorter than this is mostly pipeline fill and record traffic

struct ScorePlan {
    int row_tiles;         // ceil(rows / TILE_ROWS)
    int vocab_tiles;       // ceil(V / TILE_VOCAB)
    int splits;            // 1 .. min(vocab_tiles, MAX_SPLITS)
    int tiles_per_split;   // ceil(vocab_tiles / splits); split s walks tiles [s * tiles_per_split, min(.. + tiles_per_split, vocab_tiles))
    int stages;            // K / STAGE_K
    int workgroups;        // row_tiles * splits
    int grid;              // workgroups rounded up to a multiple of 8: the launch (surplus workgroups leave at once)
    long long workspace_bytes;   // splits * row_tiles * TILE_ROWS records
};

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

// `forced` > 0: that many splits (a test's handle), cut to what exists; 0: enough splits that row_tiles * splits reaches
// TARGET_WORKGROUPS, as long as a split keeps MIN_TILES_PER_SPLIT tiles.  Either way the count is then normalised so that no split is empty.
inline ScorePlan plan_score(int rows, int V, int K, int forced = 0) {
    ScorePlan p = {};
    if (rows <= 0 || V <= 0) return p;
    p.row_tiles = ceil_div(rows, TILE_ROWS);
    p.vocab_tiles = ceil_div(V, TILE_VOCAB);
    p.stages = K / STAGE_K;
    int want = forced > 0 ? forced : ceil_div(TARGET_WORKGROUPS, p.row_tiles);
    const int most = forced > 0 ? p.vocab_tiles : (p.vocab_tiles / MIN_TILES_PER_SPLIT > 0 ? p.vocab_tiles / MIN_TILES_PER_SPLIT : 1);
    want = want > most ? most : want;
    want = want > MAX_SPLITS ? MAX_SPLITS : want < 1 ? 1 : want;
    p.tiles_per_split = ceil_div(p.vocab_tiles, want);
    p.splits = ceil_div(p.vocab_tiles, p.tiles_per_split);
    p.workgroups = p.row_tiles * p.splits;
    p.grid = ceil_div(p.workgroups, 8) * 8;
    p.workspace_bytes = (long long)p.splits * p.row_tiles * TILE_ROWS * RECORD_BYTES;
    return p;
}

// Grid order.  Workgroups are handed to the chip's 8 dies round-robin (id % 8), each die has its own L2.  A die's share of the launch,
// ids die, die + 8, ..., is made one contiguous run of `linear` positions, and the positions walk bands of BAND_ROWS row tiles, row tile
// fastest, then the split: the 32 workgroups a die holds at once are 8 row tiles x 4 splits that start together and walk their tiles in
// step, so a stage of lm_head is fetched by one of eight and found in L2 by the other seven, and a stage of hidden by one of four.
// -> false for a surplus workgroup.
QS_SCORE_HD inline bool grid_position(const ScorePlan& p, int id, int* row_tile, int* split) {
    const int per_die = p.grid / 8;
    const int linear = (id % 8) * per_die + id / 8;
    if (linear >= p.workgroups) return false;
    const int band = linear / (BAND_ROWS * p.splits), in_band = linear - band * (BAND_ROWS * p.splits);
    const int height = p.row_tiles - band * BAND_ROWS < BAND_ROWS ? p.row_tiles - band * BAND_ROWS : BAND_ROWS;
    *split = in_band / height;
    *row_tile = band * BAND_ROWS + in_band % height;
    return true;
}

// the split whose range holds vocabulary column t (0 <= t < V)
inline int split_of_column(const ScorePlan& p, int t) { return (t / TILE_VOCAB) / p.tiles_per_split; }

}  // namespace score_plan
