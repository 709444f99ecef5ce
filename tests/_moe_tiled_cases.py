"""Grid geometries for the compute-bound grouped W4A8 tile (csrc/gemm_w4a8_moe_tiled.hip): the kernel's block -> (row block, channel
tile) walk restated, and ONE table of cases that reach what N <= 512 never does.  Pure numpy (no torch, no GPU).
tests/test_moe_tiled_grid_cpu.py proves that the restated walk visits every (row block, channel tile) once and that every case has the
geometry it claims; tests/test_moe_tiled_grid_gpu.py runs the cases.

The walk, from the kernel's header: a 1-D grid of nrb * nbn workgroups (nrb row blocks launched, nbn channel tiles) is cut into BANDS of 16
channel tiles - the last band holds what is left of nbn - and every band into GROUPS of 16 row blocks - the last group holds what is
left of nrb; inside a group the row block runs fastest.  A band of width w takes nrb * w consecutive ids, a group of height h in it
h * w.  A wrong walk computes one tile twice and another not at all: nothing faults, the missed tile keeps whatever the buffer held.

Every case runs at K = 256, the smallest the tile takes, so that its cost lies in the grid."""
import collections

import numpy as np

BAND = 16            # channel tiles of a full band
GROUP = 16           # row blocks of a full group
K = 256
X_ROWS = 40          # source rows every case gathers from


def walk(block, nrb, nbn):
    """-> (row block, channel tile) of workgroup `block` of the nrb * nbn launched."""
    band, in_band = divmod(block, nrb * BAND)
    width = min(BAND, nbn - band * BAND)
    group, in_group = divmod(in_band, GROUP * width)
    height = min(GROUP, nrb - group * GROUP)
    return group * GROUP + in_group % height, band * BAND + in_group // height


def geometry(nrb, nbn):
    """(bands, width of the last band, groups, height of the last group) of a grid."""
    bands, groups = -(-nbn // BAND), -(-nrb // GROUP)
    return bands, nbn - (bands - 1) * BAND, groups, nrb - (groups - 1) * GROUP


def true_blocks(counts, rows):
    """Row blocks of `rows` sorted rows that the experts' ranges really need; the grid launches a bound that holds for every routing."""
    return sum(-(-c // rows) for c in counts)


# counts: rows per expert.  bands .. height: what `geometry` must give; surplus: row blocks launched that no expert owns (they leave at
# once, at the end of every band)
Case = collections.namedtuple("Case", "name N counts nrb bands width groups height surplus")
CASES = [
    # a second band one tile wide; a last group one block high behind a full group
    Case("band_plus_one", 4352, (2049,), 17, 2, 1, 2, 1, 0),
    # two full bands + one tile; two full groups + 3 blocks; an empty expert, a one-row expert at the end
    Case("three_bands_ragged", 8448, (129, 0, 3840, 1), 35, 3, 1, 3, 3, 2),
    # a last band 4 tiles wide under groups that are 16 high throughout
    Case("partial_band_full_group", 5120, (2048,), 16, 2, 4, 1, 16, 0),
    # one exact band; groups of 16, 16 and 1 blocks; 24 one-row blocks
    Case("full_band_partial_groups", 4096, (1,) * 24 + (1100,), 33, 1, 16, 3, 1, 0),
]


def routing(case):
    """(expert_offsets int32 [E + 1], row_src int32 [P]): sources in [0, X_ROWS) with repeats, in no order."""
    offsets = np.concatenate([[0], np.cumsum(case.counts)]).astype(np.int32)
    P = int(offsets[-1])
    row_src = np.random.default_rng(case.N + P).integers(0, X_ROWS, size=P).astype(np.int32)
    return offsets, row_src
