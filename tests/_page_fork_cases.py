"""The fork rule of `qs_pages_fork` (include/qserve_amd.h) restated twice in numpy - a loop form and an independent array form -, a
random op-sequence generator that mixes forks into the counted op stream, and the named cases of tests/test_page_fork_gpu.py.

A STATE is a state of tests/_page_ref_cases.py (read only here, like tests/_page_cases.py) plus the pools' bytes: uint8
[L, 2, N + 1, page_bytes] - a fork is the one pool entry that moves page contents.  An OP is one of that module's, or kind "fork" with
src_rows, lengths, finished (or None).  `apply_loop` / `apply_arrays` return (new state, new finished)."""
import copy

import numpy as np

import _page_cases as P
import _page_ref_cases as R

PAGE = P.PAGE
NO_PAGES = P.NO_PAGES


def new_state(B, mb, L, N, page_bytes=256, bases=None, pool_bytes=None, seed=0):
    st = R.new_state(B, mb, L, N, page_bytes, bases)
    if pool_bytes is None:
        pool_bytes = np.random.default_rng(seed).integers(0, 256, size=(L, 2, N + 1, page_bytes), dtype=np.uint8)
    return dict(st, bytes=np.asarray(pool_bytes, np.uint8).copy())


def _need(length):
    """(w, t, need) of a source text of `length` tokens: slot length - 1 is the first one still written."""
    w, t = divmod(max(int(length), 1) - 1, PAGE)
    return w, t, w + (1 if t > 0 else 0)


def fork_loop(st, src_rows, lengths, finished=None):
    """The rule as the header words it, destination by destination."""
    N, mb, pb, count = st["N"], st["mb"], st["page_bytes"], st["count"]
    B = len(src_rows)
    fin = None if finished is None else np.asarray(finished, np.int32).copy()
    bad = not 0 <= count <= N or any(not 0 <= int(o) <= mb for o in st["owned"])
    plan = []                                                              # (d, s, w, t, need, covered)
    for d in range(B):
        s = int(src_rows[d])
        if s < 0:
            continue
        if s >= B or s == d:
            bad = True
            continue
        bad = bad or int(src_rows[s]) >= 0 or st["owned"][d] != 0
        w, t, need = _need(lengths[s])
        own_s = min(max(int(st["owned"][s]), 0), mb)
        for j in range(min(need, own_s)):
            pid = int(st["page_ids"][s, j])
            bad = bad or not 0 <= pid < N or st["refs"][pid] == 0
        plan.append((d, s, w, t, need, need <= mb and own_s >= need))
    if bad:
        return R._failed(st), fin
    S, served = 0, {}
    for d, s, w, t, need, covered in plan:
        if covered and t > 0:
            S += 1
        served[d] = covered and (t == 0 or S <= count)
    popped = min(S, count)
    for k in range(popped):
        pid = int(st["free"][count - 1 - k])
        if not 0 <= pid < N or st["refs"][pid] != 0:
            return R._failed(st), fin
    new = copy.deepcopy(st)
    slot = 0
    for d, s, w, t, need, covered in plan:
        if not served[d]:
            new["starved"][d] = 1
            if fin is not None and fin[d] == 0:
                fin[d] = NO_PAGES
            continue
        for j in range(need):
            if j < w:
                pid = int(st["page_ids"][s, j])
                new["refs"][pid] += 1
            else:
                pid = int(st["free"][count - 1 - slot])
                slot += 1
                new["refs"][pid] = 1
                if st["error"] == 0 and st["starved"][d] == 0:             # (what the copy launch reads: see the header)
                    new["bytes"][:, :, pid] = st["bytes"][:, :, int(st["page_ids"][s, w])]
            new["page_ids"][d, j] = pid
            for l in range(new["tables"].shape[0]):
                for kv in range(2):
                    new["tables"][l, d, kv, j] = st["bases"][l, kv] + pid * pb
        new["owned"][d] = need
    assert slot == popped
    new["count"] = count - popped
    return new, fin


def fork_arrays(st, src_rows, lengths, finished=None):
    """Independently: every destination at once, one cumulative sum, the popped ids as one reversed slice of the stack."""
    N, mb, pb, count = st["N"], st["mb"], st["page_bytes"], st["count"]
    src, lengths = np.asarray(src_rows, np.int64), np.asarray(lengths, np.int64)
    B = src.size
    fin = None if finished is None else np.asarray(finished, np.int32).copy()
    dst = np.nonzero(src >= 0)[0]
    s = src[dst]
    if P._broken(st, []) or bool((s >= B).any()) or bool((s == dst).any()):
        return R._failed(st), fin
    last = np.maximum(lengths[s], 1) - 1
    w, t = last // PAGE, last % PAGE
    need = w + (t > 0)
    own_s = st["owned"][s].astype(np.int64)
    cols = np.arange(mb)[None, :]
    ids = st["page_ids"][s][cols < np.minimum(need, own_s)[:, None]].astype(np.int64)
    bad = bool((src[s] >= 0).any()) or bool((st["owned"][dst] != 0).any()) or bool(((ids < 0) | (ids >= N)).any())
    bad = bad or bool((st["refs"][ids] == 0).any())
    covered = (need <= mb) & (own_s >= need)
    grow = (covered & (t > 0)).astype(np.int64)
    S = np.cumsum(grow)
    served = covered & ((grow == 0) | (S <= count))
    fresh = served & (grow > 0)
    popped = int(fresh.sum())
    stack = st["free"][:count][::-1][:popped].astype(np.int64)
    bad = bad or bool(((stack < 0) | (stack >= N)).any()) or bool((st["refs"][stack] != 0).any())
    if bad:
        return R._failed(st), fin
    new = copy.deepcopy(st)
    mat = np.where(served[:, None] & (cols < w[:, None]), st["page_ids"][s].astype(np.int64), -1)
    new["refs"] = (new["refs"] + np.bincount(mat[mat >= 0], minlength=N)).astype(np.int32)
    mat[fresh, w[fresh]] = stack[S[fresh] - 1]
    new["refs"][stack] = 1
    has = mat >= 0
    new["page_ids"][dst] = np.where(has, mat, st["page_ids"][dst])
    for kv in range(2):
        addr = st["bases"][:, kv][:, None, None] + mat[None] * pb
        new["tables"][:, dst, kv, :] = np.where(has[None], addr, st["tables"][:, dst, kv, :])
    new["owned"][dst[served]] = need[served]
    new["starved"][dst[~served]] = 1
    if fin is not None:
        refused = np.zeros((B,), bool)
        refused[dst[~served]] = True
        fin = np.where(refused & (fin == 0), NO_PAGES, fin).astype(np.int32)
    copied = fresh & (st["starved"][dst] == 0) & (st["error"] == 0)
    new["bytes"][:, :, stack[S[copied] - 1]] = st["bytes"][:, :, st["page_ids"][s[copied], w[copied]]]
    new["count"] = count - popped
    return new, fin


def apply_loop(st, op):
    if op["kind"] == "fork":
        return fork_loop(st, op["src_rows"], op["lengths"], op["finished"])
    return R.apply_loop(st, op)


def apply_arrays(st, op):
    if op["kind"] == "fork":
        return fork_arrays(st, op["src_rows"], op["lengths"], op["finished"])
    return R.apply_arrays(st, op)


def same_state(a, b):
    return R.same_state(a, b) or (None if np.array_equal(a["bytes"], b["bytes"]) else "bytes")


check_invariant = R.check_invariant
cache_after = R.cache_after


# ---- ops -------------------------------------------------------------------------------------------------------------------------------
_i32, _reserve, _poke, _unhold = P._i32, P._reserve, R._poke, R._unhold


def _fork(B, rows, lengths, finished=None):
    """rows: dict dst -> src; lengths: dict row -> length (1 elsewhere) or a full list."""
    src = np.full((B,), -1, np.int32)
    for d, s in rows.items():
        src[d] = s
    if isinstance(lengths, dict):
        full = np.ones((B,), np.int32)
        for b, n in lengths.items():
            full[b] = n
        lengths = full
    return dict(kind="fork", src_rows=src, lengths=_i32(lengths), finished=None if finished is None else _i32(finished))


def _texts(B, lens):
    """The reserve that gives row b the pages of a text of lens[b] tokens (a dict; other rows get nothing) - admission's form."""
    extra = np.zeros((B,), np.int32)
    for b, n in lens.items():
        extra[b] = n
    return _reserve(np.ones((B,), np.int32), 0, extra_rows=extra)


def random_ops(rng, B, mb, L, N, count):
    """`count` valid random ops: those of _page_ref_cases.random_ops, and forks of rows that own pages into rows that own nothing -
    several per source, several sources per launch, more often than not more than the free pages serve.  `lengths` follows what was
    reserved, so that most sources cover their fork; now and then one does not."""
    st, cache, ops = new_state(B, mb, L, N, page_bytes=8), set(), []
    lengths = rng.integers(1, 48 * mb, size=B).astype(np.int32)
    for _ in range(count):
        r = rng.random()
        live = np.nonzero(st["refs"] > 0)[0]
        if r < 0.25:
            mask = (rng.random(B) < 0.3).astype(np.int32)
            drops = [int(i) for i in sorted(cache) if rng.random() < 0.3]
            rng.shuffle(drops)
            lengths = np.where(mask != 0, 1, lengths).astype(np.int32)
            op = _unhold(mask, drops)
        elif r < 0.37 and live.size:
            rows = {}
            for b in np.nonzero(st["owned"] == 0)[0]:
                if rng.random() < 0.3:
                    rows[int(b)] = rng.choice(live, size=int(rng.integers(1, min(mb, live.size) + 1)), replace=False).tolist()
                    lengths[b] = 64 * len(rows[int(b)]) + int(rng.integers(1, 64))
            fresh = [int(i) for i in live if int(i) not in cache and rng.random() < 0.3]
            rng.shuffle(fresh)
            op = R._hold(B, mb, rows, fresh)
        elif r < 0.72 and (st["owned"] > 0).any() and (st["owned"] == 0).any():
            owners, empty = np.nonzero(st["owned"] > 0)[0], np.nonzero(st["owned"] == 0)[0]
            rows = {int(d): int(rng.choice(owners)) for d in empty if rng.random() < 0.6}
            told = lengths.copy()
            for s in set(rows.values()):                                    # (the text as far as its pages reach, at times beyond)
                reach = 64 * int(st["owned"][s])
                told[s] = reach + 1 if rng.random() < 0.2 else min(int(told[s]), reach) if rng.random() < 0.9 else reach + 70
            finished = rng.choice([0, 0, 0, 1, 2, 3], size=B).astype(np.int32) if rng.random() < 0.5 else None
            op = _fork(B, rows, told, finished)
            for d, s in rows.items():
                lengths[d] = told[s]
        else:
            extra = int(rng.choice([0, 1, 1, 1, 12, 64, 130]))
            extra_rows = np.where(rng.random(B) < 0.4, rng.integers(0, 64 * mb, size=B), 0).astype(np.int32) if rng.random() < 0.3 else None
            finished = rng.choice([0, 0, 0, 1, 2, 3], size=B).astype(np.int32) if rng.random() < 0.5 else None
            op = dict(kind="reserve", lengths=lengths.copy(), extra=extra, extra_rows=extra_rows, finished=finished)
            lengths = np.minimum(lengths + rng.integers(0, max(extra, 1) + 1, size=B), 64 * mb).astype(np.int32)
        st, _ = apply_loop(st, op)
        assert st["error"] == 0
        cache = cache_after(cache, op, False)
        ops.append(op)
    return ops


# ---- the named cases: name -> (B, mb, L, N, ops); those of BROKEN end in an op that must fail and change nothing -----------------------
B0 = (5, 4, 2, 7)
# rows 0 and 1 hold a text of 70 tokens each: row 0 has pages 0, 1, row 1 pages 2, 3; 3 pages stay free (top of the stack: 4)
_TWO = _texts(5, {0: 70, 1: 70})


def _wide(B):
    """Every third row holds a text; the two rows behind it branch off it.  N leaves pages for two thirds of the tail copies."""
    lens = {b: (37 * b) % 250 + 1 for b in range(0, B, 3)}
    rows = {d: 3 * (d // 3) for d in range(B) if d % 3}
    pages = sum(-(-n // 64) for n in lens.values())
    growers = sum(1 for d, s in rows.items() if _need(lens[s])[1] > 0)
    N = pages + 2 * growers // 3
    fin = [(b % 7 == 1) * 2 for b in range(B)]
    return B, 4, 2, N, [_texts(B, lens), _fork(B, rows, lens, fin), _unhold(_i32(np.arange(B) % 3 == 0)),
                        _reserve([lens.get(3 * (b // 3), 1) for b in range(B)], 12), _unhold(_i32(np.ones(B)))]


def named_cases():
    return {
        # len - 1 = 128: pages 0 and 1 are whole and shared, page 2 (which the source owns, empty) is not: nothing popped, nothing copied
        "t0": (*B0, [_texts(5, {0: 129}), _fork(5, {1: 0, 2: 0}, {0: 129})]),
        # len - 1 = 129: one slot of page 2 is written: shared 0 and 1, page 2 copied into the popped page 3
        "t1": (*B0, [_texts(5, {0: 130}), _fork(5, {1: 0}, {0: 130})]),
        # len - 1 = 127: page 0 shared, all but the last slot of page 1 copied
        "t63": (*B0, [_texts(5, {0: 128}), _fork(5, {3: 0}, {0: 128})]),
        # a text of one token, and lengths of 0 and below: nothing shared, nothing copied, the destination owns nothing
        "len1": (*B0, [_texts(5, {0: 1, 1: 1}), _fork(5, {2: 0, 3: 1, 4: 1}, {0: 1, 1: -5})]),
        # the destination grows behind its fork like any row, and the source's release leaves the shared page alone
        "fork_then_grow": (*B0, [_texts(5, {0: 70}), _fork(5, {1: 0}, {0: 70}), _unhold([1, 0, 0, 0, 0]), _reserve([1, 70, 1, 1, 1], 64),
                                 _unhold([0, 1, 0, 0, 0])]),
        # one source into four rows: page 0 has five holders, four tail pages popped in row order
        "one_into_many": (*B0, [_texts(5, {0: 70}), _fork(5, {1: 0, 2: 0, 3: 0, 4: 0}, {0: 70})]),
        # two sources in one launch, destinations interleaved
        "two_sources": (5, 4, 2, 9, [_texts(5, {0: 70, 3: 140}), _fork(5, {1: 0, 2: 3, 4: 3}, {0: 70, 3: 140})]),
        # 2 free pages for 4 tail copies: rows 2 and 3 are served, 4 and 5 refused, and row 6 (t = 0, asks nothing) is served behind them
        "free_ends_midway": (7, 4, 2, 7, [_texts(7, {0: 70, 1: 129}), _fork(7, {2: 0, 3: 0, 4: 0, 5: 0, 6: 1}, {0: 70, 1: 129})]),
        # the same with `finished`: row 4 becomes NO_PAGES, row 5 keeps its reason, the served rows 2 (live) and 3 (finished) keep theirs
        "free_ends_midway_finished": (7, 4, 2, 7, [_texts(7, {0: 70, 1: 129}),
                                                   _fork(7, {2: 0, 3: 0, 4: 0, 5: 0, 6: 1}, {0: 70, 1: 129}, [0, 0, 0, 2, 0, 1, 0])]),
        # a source that was refused pages (its text says 200 tokens, it owns one page), one whose text is beyond max_blocks: refused, no
        # error; row 4 branches off a source that covers and is served
        "starved_source": (*B0, [_texts(5, {0: 10, 1: 10}), _fork(5, {2: 0, 3: 1, 4: 1}, {0: 200, 1: 10}, [0] * 5),
                                 _fork(5, {2: 0}, {0: 1000})]),
        # the scans cross a wave, the workgroup's stride
        "wave": _wide(70),
        "stride": _wide(300),
        # a chunk of the row loop exactly full; the largest batch the entry takes: four chunks, the carry crosses three boundaries
        "chunk": _wide(256),
        "full": _wide(1024),
        # ---- broken invariants: the last op fails
        "source_out_of_range": (*B0, [_TWO, _fork(5, {2: 5}, {0: 70})]),
        "self_fork": (*B0, [_TWO, _fork(5, {2: 2}, {2: 1})]),
        "chained_source": (*B0, [_TWO, _fork(5, {2: 0, 3: 2}, {0: 70})]),
        # (row 1 owns exactly what the fork would give it: the copy launch's own conditions hold, only `error` stops it)
        "destination_owns_pages": (*B0, [_TWO, _fork(5, {1: 0}, {0: 70})]),
        "source_page_is_free": (*B0, [_TWO, _poke("refs", 0, 0), _fork(5, {2: 0}, {0: 70})]),
        "source_page_outside": (*B0, [_TWO, _poke("page_ids", (0, 0), 7), _fork(5, {2: 0}, {0: 70})]),
        "fork_bad_count": (*B0, [_TWO, _poke("count", None, 8), _fork(5, {2: 0}, {0: 70})]),
        "fork_bad_owned": (*B0, [_TWO, _poke("owned", 3, 5), _fork(5, {2: 0}, {0: 70})]),
        "fork_pops_a_held_page": (*B0, [_TWO, _poke("refs", 4, 1), _fork(5, {2: 0}, {0: 70})]),
    }


BROKEN = ("source_out_of_range", "self_fork", "chained_source", "destination_owns_pages", "source_page_is_free", "source_page_outside",
          "fork_bad_count", "fork_bad_owned", "fork_pops_a_held_page")
