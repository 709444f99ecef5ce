"""Case tables of the forced-geometry sweeps over the two older W4A8 decode kernels and of the W8A8 kernel: plain data and a
few pure functions (no torch, no GPU).  tests/test_gemm_family_cases_cpu.py checks, without a GPU, that every row plans as it
claims (qs_w4a8_gemm_plan) and that the tables cover what they are meant to; tests/test_gemm_decode_families_gpu.py runs them.

Selection codes (include/qserve_amd.h qs_gemm_variant_code, decoded in csrc/gemm_plan.h):
    split-K  1000 + 100 * mo + 10 * S + NW    mo = 1 .. 4: m-tiles (16 tokens each) per workgroup, XCD-aware 1-D mapping when
                                              the tokens need more than one workgroup; mo = 9: as many m-tiles as the tokens
                                              need (up to 4), classic 2-D grid.  S = blocks that split K, NW = waves.
    pair     2001                             the LDS-pair kernel wherever its preconditions hold (N % 128 == 0, K >= 256)
The planner clamps a split-K code: 8 waves become 4 at more than 2 m-tiles, 3 / 5 / 6 / 7 waves become 4, more waves than
K / 128 k-steps become 1, S and NW below 1 become 1 - so every row carries the plan it is MEANT to get, (m_tiles, waves, S,
xcd flag), and the CPU test holds the planner to it: a row that silently ran another geometry would test nothing."""

FAMILY_SPLITK, FAMILY_PAIR = 1, 2          # plan5[0] of qs_w4a8_gemm_plan
PAIR_FORCED = 2001
MODES = ("per_channel", "per_group", "per_group_any_bytes")     # the last: level-2 scales outside the protective range

# (mo, S, NW, M, N, K, (m_tiles, waves, S, xcd flag) the planner must report).  K = 128 * {1, 3, 5, 13, 17} k-steps: with 8
# waves and 2 stages a full round is 16 steps, so 13 is a partial first round and 17 a second round with one live wave.
# M: ragged last tiles, one to nine token blocks.  N = 64 * {1, 3, 8} units: 8 takes the 1-D XCD mapping, 3 cannot.
SPLITK = [
    # every m-tile override x wave count, un-split and cross-block
    (1, 1, 1,   1,  64,  128, (1, 1, 1, 0)),
    (1, 2, 1,  16, 192,  384, (1, 1, 2, 0)),
    (1, 1, 2,  33, 192, 1664, (1, 2, 1, 1)),
    (1, 3, 2,  50, 512, 2176, (1, 2, 3, 1)),
    (1, 1, 4,  65, 512, 1664, (1, 4, 1, 1)),
    (1, 4, 4, 130,  64, 2176, (1, 4, 4, 1)),
    (1, 1, 8,  16,  64, 1664, (1, 8, 1, 0)),
    (1, 2, 8,  17, 192, 2176, (1, 8, 2, 1)),
    (2, 1, 1,  50, 192, 1664, (2, 1, 1, 1)),
    (2, 3, 1,  64, 512, 2176, (2, 1, 3, 1)),
    (2, 1, 2, 130, 512, 1664, (2, 2, 1, 1)),
    (2, 4, 2,   1,  64, 2176, (2, 2, 4, 0)),
    (2, 1, 4,  17,  64,  640, (2, 4, 1, 0)),
    (2, 2, 4,  33, 192, 1664, (2, 4, 2, 1)),
    (2, 1, 8,  64, 192, 1664, (2, 8, 1, 1)),
    (2, 3, 8,  65, 512, 2176, (2, 8, 3, 1)),
    (3, 1, 1,   1, 512,  384, (3, 1, 1, 0)),
    (3, 4, 1,  16,  64,  640, (3, 1, 4, 0)),
    (3, 1, 2,  33,  64, 1664, (3, 2, 1, 0)),
    (3, 2, 2,  50, 192, 2176, (3, 2, 2, 1)),
    (3, 1, 4,  65, 192, 2176, (3, 4, 1, 1)),
    (3, 3, 4, 130, 512,  640, (3, 4, 3, 1)),
    (3, 1, 8,  16, 512, 1664, (3, 4, 1, 0)),
    (3, 4, 8,  17,  64, 2176, (3, 4, 4, 0)),
    (4, 1, 1,  50,  64, 2176, (4, 1, 1, 0)),
    (4, 2, 1,  64, 192,  128, (4, 1, 2, 0)),
    (4, 1, 2, 130, 192, 1664, (4, 2, 1, 1)),
    (4, 3, 2,   1, 512, 2176, (4, 2, 3, 0)),
    (4, 1, 4,  17, 512, 1664, (4, 4, 1, 0)),
    (4, 4, 4,  33,  64, 2176, (4, 4, 4, 0)),
    (4, 1, 8,  64,  64, 1664, (4, 4, 1, 0)),
    (4, 2, 8,  65, 192, 2176, (4, 4, 2, 1)),
    (9, 1, 1,   1, 192,  640, (1, 1, 1, 0)),
    (9, 3, 1,  16, 512, 1664, (1, 1, 3, 0)),
    (9, 1, 2,  33, 512, 1664, (3, 2, 1, 0)),
    (9, 4, 2,  50,  64, 2176, (4, 2, 4, 0)),
    (9, 1, 4,  65,  64,  640, (4, 4, 1, 0)),
    (9, 2, 4, 130, 192, 1664, (4, 4, 2, 0)),
    (9, 1, 8,  16, 192, 1664, (1, 8, 1, 0)),
    (9, 3, 8,  17, 512, 2176, (2, 8, 3, 0)),
    # 8 waves x 2 stages over 13 and 17 k-steps
    (1, 1, 8,  16,  64, 2176, (1, 8, 1, 0)),
    (2, 1, 8,  33, 192, 1664, (2, 8, 1, 1)),
    (2, 1, 8,  33, 192, 2176, (2, 8, 1, 1)),
    (1, 1, 8,  50, 512, 1664, (1, 8, 1, 1)),
    (1, 1, 8,  50, 512, 2176, (1, 8, 1, 1)),
    (9, 1, 8,  17,  64, 1664, (2, 8, 1, 0)),
    (9, 1, 8,  17,  64, 2176, (2, 8, 1, 0)),
    (2, 1, 8, 130, 512, 1664, (2, 8, 1, 1)),
    (2, 1, 8, 130, 512, 2176, (2, 8, 1, 1)),
    (2, 3, 8,  64,  64, 1664, (2, 8, 3, 1)),
    (2, 4, 8,   1, 512, 2176, (2, 8, 4, 0)),
    # cross-block ranges: empty blocks, uneven ranges
    (1, 4, 1,  17, 192,  384, (1, 1, 4, 1)),
    (2, 4, 2,  33,  64,  384, (2, 2, 4, 1)),
    (4, 4, 1,  64, 512,  384, (4, 1, 4, 0)),
    (9, 4, 2,  50, 192,  384, (4, 2, 4, 0)),
    (1, 2, 1,  16,  64,  128, (1, 1, 2, 0)),
    (3, 3, 1,  33, 192,  128, (3, 1, 3, 0)),
    (2, 3, 2,  33, 192,  640, (2, 2, 3, 1)),
    (4, 3, 4,  64, 512,  640, (4, 4, 3, 0)),
    (1, 3, 1, 130,  64,  640, (1, 1, 3, 1)),
    (3, 3, 4,  50,  64,  640, (3, 4, 3, 1)),
    (9, 3, 2,  65, 192,  640, (4, 2, 3, 0)),
    (1, 3, 4,   1,  64, 1664, (1, 4, 3, 0)),
    (4, 2, 4, 130, 192, 2176, (4, 4, 2, 1)),
    (3, 4, 2,  17, 512, 1664, (3, 2, 4, 0)),
    # token blocks, the XCD-aware 1-D mapping and its fall-backs
    (1, 1, 4, 130, 512,  640, (1, 4, 1, 1)),
    (1, 1, 2,  50, 512,  384, (1, 2, 1, 1)),
    (2, 1, 4,  65, 512, 1664, (2, 4, 1, 1)),
    (3, 1, 4, 130, 512,  640, (3, 4, 1, 1)),
    (4, 1, 2, 130, 512,  384, (4, 2, 1, 1)),
    (2, 1, 8,  64, 512, 2176, (2, 8, 1, 1)),
    (1, 1, 1,  17, 512,  128, (1, 1, 1, 1)),
    (1, 1, 4, 130, 192,  640, (1, 4, 1, 1)),
    (1, 1, 2,  50, 192,  384, (1, 2, 1, 1)),
    (2, 1, 4,  65, 192, 1664, (2, 4, 1, 1)),
    (3, 1, 4, 130, 192,  640, (3, 4, 1, 1)),
    (4, 1, 2, 130, 192,  384, (4, 2, 1, 1)),
    (2, 1, 8,  64, 192, 2176, (2, 8, 1, 1)),
    (1, 1, 1,  17, 192,  128, (1, 1, 1, 1)),
    (1, 2, 4,  50, 512,  640, (1, 4, 2, 1)),
    (2, 3, 2, 130, 512, 1664, (2, 2, 3, 1)),
    (1, 1, 4, 130,  64,  640, (1, 4, 1, 1)),
    (4, 1, 4,   1,  64,  640, (4, 4, 1, 0)),
    (4, 1, 2,  16, 192,  384, (4, 2, 1, 0)),
    (3, 2, 2,   1, 512,  640, (3, 2, 2, 0)),
    # clamped codes
    (1, 1, 3,  33, 192,  640, (1, 4, 1, 1)),
    (1, 1, 5,  33, 192,  640, (1, 4, 1, 1)),
    (1, 1, 6,  33, 192,  640, (1, 4, 1, 1)),
    (1, 1, 7,  33, 192,  640, (1, 4, 1, 1)),
    (2, 2, 6,  17,  64, 1664, (2, 4, 2, 0)),
    (3, 1, 8,  50, 512, 1664, (3, 4, 1, 1)),
    (4, 1, 8,  64, 192, 2176, (4, 4, 1, 0)),
    (4, 2, 8,  65,  64, 1664, (4, 4, 2, 1)),
    (9, 1, 8,  64,  64, 2176, (4, 4, 1, 0)),
    (9, 1, 8,  33, 512, 1664, (3, 4, 1, 0)),
    (1, 1, 4,  16,  64,  384, (1, 1, 1, 0)),
    (2, 1, 8,  33, 192,  640, (2, 1, 1, 1)),
    (1, 1, 2,   1,  64,  128, (1, 1, 1, 0)),
    (2, 2, 4,  17, 192,  384, (2, 1, 2, 0)),
    (1, 0, 4,  50, 512,  640, (1, 4, 1, 1)),
    (1, 1, 0,  16, 192,  384, (1, 1, 1, 0)),
]

# (M, N, K) under code 2001.  M: 1 .. 4 m-tiles, beyond 64 tokens several token blocks of 4; N = 128 / 384: one and three
# channel blocks (the start rotation differs between workgroups); K / 128 = 2, 3, 5, 9, 16 k-steps = 1|1, 1|2, 2|3, 4|5 (the
# 4-deep ring wraps, uneven halves) and 8|8 local steps of the two K-halves.
PAIR = [
    (  1, 384,  256),
    (  1, 128,  384),
    (  1, 384,  640),
    (  1, 128, 1152),
    ( 16, 128,  256),
    ( 16, 384,  384),
    ( 16, 128,  640),
    ( 16, 128, 2048),
    ( 23, 384,  256),
    ( 23, 128,  384),
    ( 23, 128, 1152),
    ( 23, 384, 2048),
    ( 32, 128,  256),
    ( 32, 128,  640),
    ( 32, 384, 1152),
    ( 32, 128, 2048),
    ( 40, 128,  384),
    ( 40, 384,  640),
    ( 40, 128, 1152),
    ( 40, 384, 2048),
    ( 48, 128,  256),
    ( 48, 384,  384),
    ( 48, 128,  640),
    ( 48, 384, 1152),
    ( 50, 384,  256),
    ( 50, 128,  384),
    ( 50, 384,  640),
    ( 50, 384, 2048),
    ( 64, 128,  256),
    ( 64, 384,  384),
    ( 64, 384, 1152),
    ( 64, 128, 2048),
    ( 65, 384,  256),
    ( 65, 384,  640),
    ( 65, 128, 1152),
    ( 65, 384, 2048),
    (200, 384,  384),
    (200, 128,  640),
    (200, 384, 1152),
    (200, 128, 2048),
]

# what a tensor-parallel prefill of more than 1024 tokens runs on narrow shards: pair by the dispatcher's own choice (code -1)
PAIR_PREFILL = [(1100, 384, 256), (1100, 768, 512)]

# the dispatcher's own route (code -1) at small shapes: (M, N, K) -> (family, p0 .. p3) (None: not pinned)
OWN_ROUTE = [
    ((50, 512, 512), (FAMILY_SPLITK, 1, 4, 1, 1)),      # short K at a decode batch: 16-token workgroups, XCD mapping
    ((1100, 384, 256), (FAMILY_PAIR, None, None, None, None)),
    ((1100, 768, 512), (FAMILY_PAIR, None, None, None, None)),
    ((40, 192, 1280), (FAMILY_SPLITK, 3, 4, 1, 0)),     # three units, K / 64 = 20: no ring geometry fits
]

# qs_set_gemm_epilogue(1), the fmaf per-channel epilogue, where no other test takes it: (code, M, N, K, family, p0 .. p3) - the
# pair kernel below 4 m-tiles, and a split-K block that arrives last and finishes for the others (S = 2)
EPILOGUE_FMA = [
    (PAIR_FORCED, 23, 384, 640, (FAMILY_PAIR, None, None, None, None)),
    (1000 + 100 * 2 + 10 * 2 + 4, 130, 512, 640, (FAMILY_SPLITK, 2, 4, 2, 1)),
]

# W8A8 (M, N, K): one wave per 16 channels, four waves per workgroup - N = 16, 80 and 208 are 1, 5 and 13 waves, so the last
# workgroup has idle waves that must return (w8a8_idle_waves); M ragged in the last 64-token block
W8A8 = [(1, 16, 64), (63, 80, 192), (64, 64, 64), (65, 16, 256), (130, 208, 128), (37, 96, 256)]

SLAB_BYTES = 48 << 20          # the split-K workspace (csrc/gemm_w4a8.hip get_workspace)
MAX_TILES = 65535              # its arrival counters, the last one being the error word


def splitk_code(mo, S, NW):
    return 1000 + 100 * mo + 10 * S + NW


def splitk_grid(row):
    """(64-channel units, token blocks) of a split-K row's launch."""
    M, N, mt = row[3], row[4], row[6][0]
    return N // 64, (M + 16 * mt - 1) // (16 * mt)


def splitk_runs_xcd_mapping(row):
    """The launcher takes the planner's XCD flag only for several token blocks over a multiple of 8 units, un-split."""
    gx, gy = splitk_grid(row)
    _, _, S, xcd = row[6]
    return bool(xcd) and gy > 1 and gx % 8 == 0 and S == 1


def splitk_block_steps(row):
    """k-steps of each of the S blocks (floor boundaries, as the kernel cuts them)."""
    n, S = row[5] // 128, row[6][2]
    return [n * (z + 1) // S - n * z // S for z in range(S)]


def splitk_slab_bytes(row):
    gx, gy = splitk_grid(row)
    mt, _, S, _ = row[6]
    return gx * gy * S * mt * 4 * 64 * 16


def pair_m_tiles(M):
    return 1 if M <= 16 else 2 if M <= 32 else 3 if M <= 48 else 4


def pair_local_steps(K):
    """k-steps of the two K-halves."""
    n = K // 128
    return n // 2, n - n // 2


def w8a8_idle_waves(N):
    return -(N // 16) % 4
