"""The page pool rules of `qs_pages_reserve` / `qs_pages_release` (include/qserve_amd.h) restated twice in numpy - a row-by-row loop and
an independent array form -, the pool's invariant, a random op-sequence generator and the named cases of tests/test_page_pool_gpu.py.

A STATE is a dict of numpy arrays: free int32 [N], count (int), page_ids int32 [B, mb], owned / starved int32 [B], error (int), tables
int64 [L, B, 2, mb], bases int64 [L, 2], and the constants N, mb, page_bytes.  An OP is a dict: kind "reserve" with lengths, extra,
extra_rows (or None), finished (or None; the restatements return the updated copy under the same key) - or kind "release" with mask.
`apply_loop` / `apply_arrays` return (new state, new finished)."""
import copy

import numpy as np

NO_PAGES = 3
PAGE = 64


def new_state(B, mb, L, N, page_bytes=256, bases=None):
    """The state paging.PagePool starts from: every page free, page 0 on top of the stack, every table entry the sink."""
    if bases is None:
        bases = np.array([[(2 * l + kv + 1) << 32 for kv in range(2)] for l in range(L)], np.int64)
    bases = np.asarray(bases, np.int64).reshape(L, 2)
    tables = np.broadcast_to((bases + N * page_bytes)[:, None, :, None], (L, B, 2, mb)).copy()
    return dict(free=np.arange(N - 1, -1, -1, dtype=np.int32), count=N, page_ids=np.full((B, mb), -1, np.int32), owned=np.zeros((B,), np.int32),
                starved=np.zeros((B,), np.int32), error=0, tables=tables, bases=bases, N=N, mb=mb, page_bytes=page_bytes)


def _broken(st, ids):
    return not 0 <= st["count"] <= st["N"] or bool(((st["owned"] < 0) | (st["owned"] > st["mb"])).any()) or \
        any(not 0 <= int(i) < st["N"] for i in ids)


def _need(length, e, mb):
    return min((max(int(length), 1) - 1 + max(int(e), 0) + PAGE - 1) // PAGE, mb)


def reserve_loop(st, lengths, extra, extra_rows=None, finished=None):
    """The rule as the header words it, row by row."""
    st = copy.deepcopy(st)
    fin = None if finished is None else finished.copy()
    N, mb, pb, count = st["N"], st["mb"], st["page_bytes"], st["count"]
    B = len(lengths)
    grows, S, run = [], [], 0
    for b in range(B):
        e = extra if extra_rows is None else max(int(extra_rows[b]), 0)
        own = min(max(int(st["owned"][b]), 0), mb)
        g = 0 if (fin is not None and fin[b] != 0) else max(_need(lengths[b], e, mb) - own, 0)
        run += g
        grows.append(g)
        S.append(run)
    served = [S[b] <= count for b in range(B)]
    popped = max([S[b] for b in range(B) if served[b]] + [0])
    ids = [st["free"][min(max(count, 0), N) - 1 - s] for s in range(min(popped, N))]
    if _broken(st, ids):
        st["error"] = 1
        return st, fin
    for b in range(B):
        if grows[b] == 0:
            continue
        if served[b]:
            for j in range(grows[b]):
                pid = int(st["free"][count - 1 - (S[b] - grows[b] + j)])
                col = int(st["owned"][b]) + j
                st["page_ids"][b, col] = pid
                for l in range(st["tables"].shape[0]):
                    for kv in range(2):
                        st["tables"][l, b, kv, col] = st["bases"][l, kv] + pid * pb
            st["owned"][b] += grows[b]
        else:
            st["starved"][b] = 1
            if fin is not None and fin[b] == 0:
                fin[b] = NO_PAGES
    st["count"] = count - popped
    return st, fin


def reserve_arrays(st, lengths, extra, extra_rows=None, finished=None):
    """Independently: whole-batch arrays, one cumulative sum, the popped ids as one reversed slice of the stack."""
    st = copy.deepcopy(st)
    fin = None if finished is None else finished.copy()
    N, mb, pb, count = st["N"], st["mb"], st["page_bytes"], st["count"]
    lengths = np.asarray(lengths, np.int64)
    e = np.full(lengths.shape, extra, np.int64) if extra_rows is None else np.maximum(np.asarray(extra_rows, np.int64), 0)
    need = np.minimum(-(-(np.maximum(lengths, 1) - 1 + e) // PAGE), mb)
    own = np.clip(st["owned"].astype(np.int64), 0, mb)
    grow = np.maximum(need - own, 0)
    if fin is not None:
        grow = np.where(fin != 0, 0, grow)
    S = np.cumsum(grow)
    served = S <= count
    popped = int(S[served].max()) if served.any() else 0
    top = min(max(count, 0), N)
    stack = st["free"][:top][::-1][:popped]                              # stack[s]: the page of popped slot s
    if _broken(st, stack):
        st["error"] = 1
        return st, fin
    take = served & (grow > 0)
    rows = np.repeat(np.arange(len(lengths)), np.where(take, grow, 0))
    slot = np.arange(popped)
    cols = own[rows] + slot - (S - grow)[rows]
    st["page_ids"][rows, cols] = stack
    for kv in range(2):
        st["tables"][:, rows, kv, cols] = st["bases"][:, kv][:, None] + stack.astype(np.int64)[None, :] * pb
    st["owned"] = (own + np.where(take, grow, 0)).astype(np.int32)
    refused = ~served & (grow > 0)
    st["starved"] = np.where(refused, 1, st["starved"]).astype(np.int32)
    if fin is not None:
        fin = np.where(refused & (fin == 0), NO_PAGES, fin).astype(np.int32)
    st["count"] = count - popped
    return st, fin


def release_loop(st, mask):
    st = copy.deepcopy(st)
    N, mb, pb, count = st["N"], st["mb"], st["page_bytes"], st["count"]
    B = len(mask)
    ids = [st["page_ids"][b, j] for b in range(B) if mask[b] != 0 for j in range(min(max(int(st["owned"][b]), 0), mb))]
    if _broken(st, ids) or count + len(ids) > N:
        st["error"] = 1
        return st
    at = count
    for b in range(B):
        if mask[b] == 0:
            continue
        for j in range(int(st["owned"][b])):
            st["free"][at] = st["page_ids"][b, j]
            at += 1
            st["page_ids"][b, j] = -1
            for l in range(st["tables"].shape[0]):
                for kv in range(2):
                    st["tables"][l, b, kv, j] = st["bases"][l, kv] + N * pb
        st["owned"][b] = 0
        st["starved"][b] = 0
    st["count"] = at
    return st


def release_arrays(st, mask):
    st = copy.deepcopy(st)
    N, mb, pb, count = st["N"], st["mb"], st["page_bytes"], st["count"]
    m = np.asarray(mask) != 0
    held = (np.arange(mb)[None, :] < np.clip(st["owned"], 0, mb)[:, None]) & m[:, None]     # row-major: row order, then logical page order
    ids = st["page_ids"][held]
    if _broken(st, ids) or count + ids.size > N:
        st["error"] = 1
        return st
    st["free"][count:count + ids.size] = ids
    st["page_ids"][held] = -1
    sink = (st["bases"] + N * pb)[:, None, :, None]
    st["tables"] = np.where(held[None, :, None, :], sink, st["tables"])
    st["owned"] = np.where(m, 0, st["owned"]).astype(np.int32)
    st["starved"] = np.where(m, 0, st["starved"]).astype(np.int32)
    st["count"] = count + int(ids.size)
    return st


def apply_loop(st, op):
    if op["kind"] == "reserve":
        return reserve_loop(st, op["lengths"], op["extra"], op["extra_rows"], op["finished"])
    return release_loop(st, op["mask"]), None


def apply_arrays(st, op):
    if op["kind"] == "reserve":
        return reserve_arrays(st, op["lengths"], op["extra"], op["extra_rows"], op["finished"])
    return release_arrays(st, op["mask"]), None


def same_state(a, b):
    """The first key under which two states differ, or None."""
    for k in ("free_live", "count", "page_ids", "owned", "starved", "error", "tables"):
        if k == "free_live":                                              # (entries above count are not part of the state ...
            if a["count"] != b["count"] or not np.array_equal(a["free"][:max(a["count"], 0)], b["free"][:max(b["count"], 0)]):
                return k
        elif not np.array_equal(a[k], b[k]):
            return k
    return None if np.array_equal(a["free"], b["free"]) else "free"       # ... but both forms and the kernel leave them alike anyway)


def check_invariant(st):
    """set(free[:count]) and {page_ids >= 0} are disjoint and together {0 .. N-1}; owned pages are a row's first columns; the tables name
    exactly those pages, the sink elsewhere."""
    N, mb, pb = st["N"], st["mb"], st["page_bytes"]
    assert st["error"] == 0 and 0 <= st["count"] <= N
    free = st["free"][:st["count"]].tolist()
    held = st["page_ids"][st["page_ids"] >= 0].tolist()
    assert len(set(free)) == len(free) and len(set(held)) == len(held) and not set(free) & set(held)
    assert set(free) | set(held) == set(range(N))
    has = st["page_ids"] >= 0
    assert np.array_equal(has, np.arange(mb)[None, :] < st["owned"][:, None])
    ids = np.where(has, st["page_ids"], N).astype(np.int64)
    want = st["bases"][:, None, :, None] + ids[None, :, None, :] * pb
    assert np.array_equal(st["tables"], want)


def random_ops(rng, B, mb, count, with_finished=True):
    """`count` random ops over one evolving text length per row: steps, trees, prompts through extra_rows, finished masks, releases -
    demand is often above what is free."""
    lengths = rng.integers(1, 40, size=B).astype(np.int32)
    ops = []
    for _ in range(count):
        r = rng.random()
        if r < 0.3:
            mask = (rng.random(B) < 0.3).astype(np.int32)
            lengths = np.where(mask != 0, 1, lengths).astype(np.int32)
            ops.append(dict(kind="release", mask=mask))
            continue
        extra = int(rng.choice([0, 1, 1, 1, 12, 64, 130]))
        extra_rows = None
        if r < 0.45:
            extra_rows = np.where(rng.random(B) < 0.4, rng.integers(0, 64 * mb, size=B), 0).astype(np.int32)
        finished = None
        if with_finished and rng.random() < 0.5:
            finished = rng.choice([0, 0, 0, 1, 2, 3], size=B).astype(np.int32)
        ops.append(dict(kind="reserve", lengths=lengths.copy(), extra=extra, extra_rows=extra_rows, finished=finished))
        lengths = np.minimum(lengths + rng.integers(0, max(extra, 1) + 1, size=B), 64 * mb).astype(np.int32)
    return ops


# ---- the named cases: (B, mb, L, N, ops) -------------------------------------------------------------------------------------------
def _i32(v):
    return np.asarray(v, np.int32)


def _reserve(lengths, extra, extra_rows=None, finished=None):
    return dict(kind="reserve", lengths=_i32(lengths), extra=extra, extra_rows=None if extra_rows is None else _i32(extra_rows),
                finished=None if finished is None else _i32(finished))


def _release(mask):
    return dict(kind="release", mask=_i32(mask))


BOUNDARY = [64, 65, 1, 128, 129]                                          # needs at extra = 1: 1, 2, 1, 2, 3; at extra = 12: 2, 2, 1, 3, 3


def named_cases():
    wide = lambda B: _i32([(37 * b) % 200 + 1 for b in range(B)])         # noqa: E731
    return {
        # 9 pages wanted, 7 there: rows 0 .. 3 take 6, row 4 (3 pages) starves although 1 is left
        "step": (5, 4, 2, 7, [_reserve(BOUNDARY, 1)]),
        # 11 wanted: rows 0 .. 2 take 5, row 3 (3 pages) starves at 8 > 7, and row 4 with it
        "tree12": (5, 4, 2, 7, [_reserve(BOUNDARY, 12)]),
        # a middle row starves: 2 pages are left, row 1 wants 3; rows 2 and 3 want nothing and keep going, row 4 wants 1 and is refused
        "middle_starves": (5, 4, 2, 7, [_reserve([1, 1, 10, 10, 10], 1), _reserve([60, 200, 11, 11, 65], 1)]),
        # a finished row does not grow (row 1 would have taken 4) and keeps its reason; rows 3 and 4 starve and become NO_PAGES
        "finished_mask": (5, 4, 2, 7, [_reserve([250, 256, 100, 256, 1], 1, finished=[0, 2, 0, 0, 0])]),
        # release rows 1 and 3, reserve again: the pages come back in the order they were pushed, last pushed first
        "release_reuse": (5, 4, 2, 7, [_reserve([64, 128, 1, 100, 1], 1), _release([0, 1, 0, 1, 0]), _reserve([64, 1, 190, 1, 70], 1),
                                       _release([1, 1, 1, 1, 1]), _reserve(BOUNDARY, 1)]),
        # admission's form: lengths = 1 and the prompt in extra_rows, 0 elsewhere; 6 wanted of 5: rows 1 and 3 are served, row 4 is not
        "extra_rows": (5, 4, 2, 7, [_reserve([100, 1, 1, 1, 1], 0, extra_rows=[1, 0, 0, 0, 0]),
                                    _reserve([1, 1, 1, 1, 1], 0, extra_rows=[0, 130, 0, 64, 65])]),
        # the scan crosses a wave, the workgroup's stride
        "wave": (70, 4, 2, 150, [_reserve(wide(70), 1), _release(_i32(np.arange(70) % 3 == 0)), _reserve(wide(70) + 60, 12)]),
        "stride": (300, 4, 2, 700, [_reserve(wide(300), 1), _release(_i32(np.arange(300) % 3 == 1)), _reserve(wide(300) + 60, 12)]),
        # a chunk of the row loop exactly full; the largest batch the entries take: four chunks, the carry crosses three boundaries
        "chunk": (256, 4, 2, 600, [_reserve(wide(256), 1), _release(_i32(np.arange(256) % 3 == 1)), _reserve(wide(256) + 60, 12)]),
        "full": (1024, 4, 2, 2400, [_reserve(wide(1024), 1), _release(_i32(np.arange(1024) % 3 == 1)), _reserve(wide(1024) + 60, 12)]),
    }
