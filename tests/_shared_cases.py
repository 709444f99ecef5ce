"""Case builders of the shared-prefix append attention tests (tests/test_append_shared_cpu.py, tests/test_append_shared_gpu.py).

A batch is cut into groups of batch-adjacent sequences; group g shares `prefix[g]` leading cached tokens (whole 64-token pages).  Every
sequence is FILLED through a table of its own (`own`: scattered blocks, nothing shared - each member holds its own, DIFFERENT bytes
at the prefix positions); `aliased` points the members' entries below prefix / 64 at the first member's blocks.  The expected values
are `_append_cases.expected` on the ALIASED tables; the `own` tables serve as the decoy of the "sharing is real" test: valid quantised
pages with finite scales that a kernel reading a member's own prefix entries would pick up."""
import numpy as np

from _append_cases import scattered_tables

BN = 64

# the ragged batch of the issue: sizes 5 / 1 / 3, prefixes 192 / 0 / 64, member pasts prefix + {0, 1, 63, 64, 130}, n in {0, 1, 7, 13, 20}
SIZES = (5, 1, 3)
PREFIXES = (192, 0, 64)
EXTRAS = (0, 1, 63, 64, 130, 63, 0, 64, 130)
NS = (7, 0, 13, 1, 20, 13, 20, 0, 7)


def layout(sizes, prefixes, extras, ns):
    """-> dict(group_offsets [groups + 1], seq_group [B], pasts [B], cu_q [B + 1], group_tokens [groups]) (numpy int32)."""
    assert len(sizes) == len(prefixes) and sum(sizes) == len(extras) == len(ns) and all(p % BN == 0 for p in prefixes)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    seq_group = np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)
    pasts = np.asarray([prefixes[g] + e for g, e in zip(seq_group, extras)], np.int32)
    cu_q = np.concatenate([[0], np.cumsum(ns)]).astype(np.int32)
    group_tokens = np.asarray([cu_q[offs[g + 1]] - cu_q[offs[g]] for g in range(len(sizes))], np.int32)
    return dict(group_offsets=offs, seq_group=seq_group, pasts=pasts, cu_q=cu_q, group_tokens=group_tokens,
                prefix_lens=np.asarray(prefixes, np.int32))


def alias(own, group_offsets, prefixes):
    """own int64 [B, 2, mb] -> a copy whose entries < prefix / 64 of every member (K and V) are the group's first member's."""
    t = own.copy()
    for g, p in enumerate(prefixes):
        f, e = int(group_offsets[g]), int(group_offsets[g + 1])
        t[f:e, :, : p // BN] = own[f:f + 1, :, : p // BN]
    return t


def tables_for(rng, lay, ns, spare=3):
    """-> (own, aliased, nblocks, mb): scattered tables with room for past + n tokens and one more page per sequence."""
    mb = int(max(p + n for p, n in zip(lay["pasts"], ns)) + BN - 1) // BN + 1
    own, nblocks = scattered_tables(rng, len(ns), mb, spare)
    return own, alias(own, lay["group_offsets"], lay["prefix_lens"]), nblocks, mb


def split_range(tokens, split, splits):
    """The kernels' page range of `split` of `splits` over `tokens` cached tokens -> (first page, pages); ceil-sized."""
    np_all = -(-tokens // BN)
    pps = -(-np_all // splits)
    p0 = min(split * pps, np_all)
    return p0, min(pps, np_all - p0)
