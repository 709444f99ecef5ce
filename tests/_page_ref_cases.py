"""The reference-count rules of `qs_pages_reserve_refs` / `qs_pages_hold` / `qs_pages_unhold` (include/qserve_amd.h) restated twice in
numpy - a loop form and an independent array form -, the counted pool's invariant, a random op-sequence generator and the named cases
of tests/test_page_refs_gpu.py.

A STATE is a state of tests/_page_cases.py (read only here) plus refs int32 [N].  An OP is a dict: kind "reserve" (as there), kind
"hold" with take, src, hold_ids - kind "unhold" with mask, drop_ids - or kind "poke" with key, at, value: the state is corrupted by
hand, for the broken invariants no launch can reach.  `apply_loop` / `apply_arrays` return (new state, new finished).  The holds of the
prefix cache are no part of the state: `cache_after` follows them through the ops, for the invariant."""
import copy
from collections import Counter

import numpy as np

import _page_cases as P


def new_state(B, mb, L, N, page_bytes=256, bases=None):
    return dict(P.new_state(B, mb, L, N, page_bytes, bases), refs=np.zeros((N,), np.int32))


def _failed(st):
    st = copy.deepcopy(st)
    st["error"] = 1
    return st


def _popped(before, after):
    """The ids a reserve popped, top of the stack first."""
    return before["free"][after["count"]:before["count"]][::-1]


# ---- reserve: the uncounted rule, and refs = 1 on what was popped ----------------------------------------------------------------------
def reserve_loop(st, lengths, extra, extra_rows=None, finished=None):
    new, fin = P.reserve_loop(st, lengths, extra, extra_rows, finished)
    if new["error"]:
        return new, fin
    for pid in _popped(st, new):
        if st["refs"][pid] != 0:
            return _failed(st), (None if finished is None else finished.copy())
        new["refs"][pid] = 1
    return new, fin


def reserve_arrays(st, lengths, extra, extra_rows=None, finished=None):
    new, fin = P.reserve_arrays(st, lengths, extra, extra_rows, finished)
    if new["error"]:
        return new, fin
    ids = _popped(st, new)
    if st["refs"][ids].any():
        return _failed(st), (None if finished is None else finished.copy())
    new["refs"][ids] = 1
    return new, fin


# ---- hold ------------------------------------------------------------------------------------------------------------------------------
def hold_loop(st, take, src, hold_ids):
    N, mb, pb = st["N"], st["mb"], st["page_bytes"]
    bad, seen = False, set()
    for b in range(len(take)):
        t = int(take[b])
        bad = bad or not 0 <= t <= mb or (t > 0 and st["owned"][b] != 0)
        for j in range(min(max(t, 0), mb)):
            pid = int(src[b, j])
            bad = bad or not 0 <= pid < N or st["refs"][pid] == 0
    for pid in (int(i) for i in hold_ids):
        bad = bad or not 0 <= pid < N or st["refs"][pid] == 0 or pid in seen
        seen.add(pid)
    if bad:
        return _failed(st)
    st = copy.deepcopy(st)
    for b in range(len(take)):
        for j in range(int(take[b])):
            pid = int(src[b, j])
            st["page_ids"][b, j] = pid
            for l in range(st["tables"].shape[0]):
                for kv in range(2):
                    st["tables"][l, b, kv, j] = st["bases"][l, kv] + pid * pb
            st["refs"][pid] += 1
        if take[b] > 0:
            st["owned"][b] = take[b]
    for pid in hold_ids:
        st["refs"][int(pid)] += 1
    return st


def hold_arrays(st, take, src, hold_ids):
    N, mb, pb = st["N"], st["mb"], st["page_bytes"]
    take, src, hold_ids = np.asarray(take, np.int64), np.asarray(src, np.int64), np.asarray(hold_ids, np.int64).reshape(-1)
    named = np.arange(mb)[None, :] < np.clip(take, 0, mb)[:, None]
    ids = np.concatenate((src[named], hold_ids))
    bad = bool(((take < 0) | (take > mb) | ((take > 0) & (st["owned"] != 0))).any()) or bool(((ids < 0) | (ids >= N)).any())
    bad = bad or bool((st["refs"][ids] == 0).any()) or np.unique(hold_ids).size != hold_ids.size
    if bad:
        return _failed(st)
    st = copy.deepcopy(st)
    st["page_ids"][named] = src[named]
    for kv in range(2):
        addr = st["bases"][:, kv][:, None, None] + src[None, :, :] * pb
        st["tables"][:, :, kv, :] = np.where(named[None], addr, st["tables"][:, :, kv, :])
    st["owned"] = np.where(take > 0, take, st["owned"]).astype(np.int32)
    st["refs"] = (st["refs"] + np.bincount(ids, minlength=N)).astype(np.int32)
    return st


# ---- unhold ----------------------------------------------------------------------------------------------------------------------------
def unhold_loop(st, mask, drop_ids):
    N, mb, pb, count = st["N"], st["mb"], st["page_bytes"], st["count"]
    B = len(mask)
    H = [int(st["page_ids"][b, j]) for b in range(B) if mask[b] != 0 for j in range(min(max(int(st["owned"][b]), 0), mb))]
    H += [int(i) for i in drop_ids]
    if P._broken(st, H):
        return _failed(st)
    g = Counter(H)
    if any(n > st["refs"][pid] for pid, n in g.items()):
        return _failed(st)
    freed = []
    for pid in H:                                                           # (first occurrences, in the order of H)
        if g[pid] == st["refs"][pid] and pid not in freed:
            freed.append(pid)
    if count + len(freed) > N:
        return _failed(st)
    st = copy.deepcopy(st)
    for pid, n in g.items():
        st["refs"][pid] -= n
    for i, pid in enumerate(freed):
        st["free"][count + i] = pid
    for b in range(B):
        if mask[b] == 0:
            continue
        for j in range(int(st["owned"][b])):
            st["page_ids"][b, j] = -1
            for l in range(st["tables"].shape[0]):
                for kv in range(2):
                    st["tables"][l, b, kv, j] = st["bases"][l, kv] + N * pb
        st["owned"][b] = st["starved"][b] = 0
    st["count"] = count + len(freed)
    return st


def unhold_arrays(st, mask, drop_ids):
    N, mb, pb, count = st["N"], st["mb"], st["page_bytes"], st["count"]
    m = np.asarray(mask) != 0
    held = (np.arange(mb)[None, :] < np.clip(st["owned"], 0, mb)[:, None]) & m[:, None]
    H = np.concatenate((st["page_ids"][held].astype(np.int64), np.asarray(drop_ids, np.int64).reshape(-1)))
    if P._broken(st, H):
        return _failed(st)
    g = np.bincount(H, minlength=N)
    if (g > st["refs"]).any():
        return _failed(st)
    ids, first = np.unique(H, return_index=True)
    ids, first = ids[g[ids] == st["refs"][ids]], first[g[ids] == st["refs"][ids]]
    freed = ids[np.argsort(first)]
    if count + freed.size > N:
        return _failed(st)
    st = copy.deepcopy(st)
    st["refs"] = (st["refs"] - g).astype(np.int32)
    st["free"][count:count + freed.size] = freed
    st["page_ids"][held] = -1
    st["tables"] = np.where(held[None, :, None, :], (st["bases"] + N * pb)[:, None, :, None], st["tables"])
    st["owned"] = np.where(m, 0, st["owned"]).astype(np.int32)
    st["starved"] = np.where(m, 0, st["starved"]).astype(np.int32)
    st["count"] = count + int(freed.size)
    return st


def poke(st, key, at, value):
    st = copy.deepcopy(st)
    if key in ("count", "error"):
        st[key] = int(value)
    else:
        st[key][at] = value
    return st


def _apply(st, op, reserve, hold, unhold):
    if op["kind"] == "reserve":
        return reserve(st, op["lengths"], op["extra"], op["extra_rows"], op["finished"])
    if op["kind"] == "hold":
        return hold(st, op["take"], op["src"], op["hold_ids"]), None
    if op["kind"] == "unhold":
        return unhold(st, op["mask"], op["drop_ids"]), None
    return poke(st, op["key"], op["at"], op["value"]), None


def apply_loop(st, op):
    return _apply(st, op, reserve_loop, hold_loop, unhold_loop)


def apply_arrays(st, op):
    return _apply(st, op, reserve_arrays, hold_arrays, unhold_arrays)


def cache_after(cache, op, failed):
    """The cache's holds (a set of ids) behind an op that did not fail."""
    if failed or op["kind"] not in ("hold", "unhold"):
        return set(cache)
    return set(cache) | set(int(i) for i in op["hold_ids"]) if op["kind"] == "hold" else set(cache) - set(int(i) for i in op["drop_ids"])


def same_state(a, b):
    return P.same_state(a, b) or (None if np.array_equal(a["refs"], b["refs"]) else "refs")


def check_invariant(st, cache=()):
    """refs[id] = the (row, column) entries of page_ids that name id + 1 if the cache holds it; a page is on the stack, once, iff its
    count is 0; owned pages are a row's first columns; the tables name exactly page_ids, the sink elsewhere."""
    N, mb, pb = st["N"], st["mb"], st["page_bytes"]
    assert st["error"] == 0 and 0 <= st["count"] <= N
    named = st["page_ids"][st["page_ids"] >= 0]
    assert ((named >= 0) & (named < N)).all()
    want = np.bincount(named, minlength=N) + np.bincount(np.asarray(sorted(cache), np.int64), minlength=N)
    assert np.array_equal(st["refs"], want), (st["refs"], want)
    free = st["free"][:st["count"]].tolist()
    assert len(set(free)) == len(free) and set(free) == set(np.nonzero(st["refs"] == 0)[0].tolist())
    has = st["page_ids"] >= 0
    assert np.array_equal(has, np.arange(mb)[None, :] < st["owned"][:, None])
    ids = np.where(has, st["page_ids"], N).astype(np.int64)
    assert np.array_equal(st["tables"], st["bases"][:, None, :, None] + ids[None, :, None, :] * pb)


# ---- ops -------------------------------------------------------------------------------------------------------------------------------
_i32 = P._i32
_reserve = P._reserve


def _hold(B, mb, rows, hold_ids=()):
    take, src = np.zeros((B,), np.int32), np.zeros((B, mb), np.int32)
    for b, ids in rows.items():
        take[b] = len(ids)
        src[b, :min(len(ids), mb)] = ids[:mb]
    return dict(kind="hold", take=take, src=src, hold_ids=_i32(list(hold_ids)))


def _unhold(mask, drop_ids=()):
    return dict(kind="unhold", mask=_i32(mask), drop_ids=_i32(list(drop_ids)))


def _poke(key, at, value):
    return dict(kind="poke", key=key, at=at, value=value)


def random_ops(rng, B, mb, L, N, count):
    """`count` valid random ops - counted reserves as in _page_cases.random_ops, holds of live pages into rows that own nothing (the
    same page often into several rows), cache holds and drops, unholds of random rows - made by following the loop restatement."""
    st, cache, ops = new_state(B, mb, L, N), set(), []
    lengths = rng.integers(1, 40, size=B).astype(np.int32)
    for _ in range(count):
        r = rng.random()
        live = np.nonzero(st["refs"] > 0)[0]
        if r < 0.25:
            mask = (rng.random(B) < 0.3).astype(np.int32)
            drops = [int(i) for i in sorted(cache) if rng.random() < 0.3]
            rng.shuffle(drops)
            lengths = np.where(mask != 0, 1, lengths).astype(np.int32)
            op = _unhold(mask, drops)
        elif r < 0.5 and live.size:
            rows = {}
            for b in np.nonzero(st["owned"] == 0)[0]:
                if rng.random() < 0.5:
                    rows[int(b)] = rng.choice(live, size=int(rng.integers(1, min(mb, live.size) + 1)), replace=False).tolist()
                    lengths[b] = 64 * len(rows[int(b)]) + int(rng.integers(1, 64))
            fresh = [int(i) for i in live if int(i) not in cache and rng.random() < 0.3]
            rng.shuffle(fresh)
            op = _hold(B, mb, rows, fresh)
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


def unshared_ops(rng, B, mb, count):
    """_page_cases.random_ops in this module's words (release -> unhold without drops): what a counted pool that never shares runs."""
    return [op if op["kind"] == "reserve" else _unhold(op["mask"]) for op in P.random_ops(rng, B, mb, count)]


# ---- the named cases: name -> (B, mb, L, N, ops); those of BROKEN end in an op that must fail and change nothing -----------------------
B0 = (5, 4, 2, 7)
# rows 0 and 1 take 2 pages each: row 0 has pages 0, 1, row 1 pages 2, 3; 3 pages stay free (top of the stack: 4)
_TWO = _reserve([1, 1, 1, 1, 1], 0, extra_rows=[100, 100, 0, 0, 0])


def _wide_ops(B, N):
    """Every third row lets go and maps two pages of other rows instead (many rows the same ones), the cache holds every third live
    page; rows let go, the rest grows behind what it holds; at the end everything is given up, the cache's holds in reverse."""
    wide = _i32([(37 * b) % 200 + 1 for b in range(B)])
    ops = [_reserve(wide, 1), _unhold(_i32(np.arange(B) % 3 == 1))]
    st = new_state(B, 4, 2, N)
    for op in ops:
        st, _ = apply_loop(st, op)
    live = np.nonzero(st["refs"] > 0)[0]
    rows = {b: [int(live[(b * 7 + j) % live.size]) for j in range(2)] for b in range(1, B, 3)}
    cached = [int(i) for i in live[::3]]
    return ops + [_hold(B, 4, rows, cached), _unhold(_i32(np.arange(B) % 3 == 0)), _reserve(wide + 60, 12),
                  _unhold(_i32(np.ones(B)), cached[::-1])]


def named_cases():
    return {
        # page 0 into rows 2, 3, 4 by one hold: refs[0] = 4
        "three_rows": (*B0, [_TWO, _hold(5, 4, {2: [0], 3: [0], 4: [0, 1]})]),
        # rows 2 and 3 share page 2 and nothing else holds it once row 1 lets go: pushed once, where row 1 named it first
        "shared_released_together": (*B0, [_TWO, _hold(5, 4, {2: [2], 3: [3, 2]}), _unhold([0, 1, 1, 1, 0])]),
        # one of two holders lets go: nothing is pushed
        "one_of_two": (*B0, [_TWO, _hold(5, 4, {2: [0, 1]}), _unhold([0, 0, 1, 0, 0]), _unhold([1, 0, 0, 0, 0])]),
        # the cache holds pages 0 and 1, drops them while row 0 holds them (nothing pushed), then the row lets go (both pushed)
        "cache_drops_first": (*B0, [_TWO, _hold(5, 4, {}, [1, 0]), _unhold([0] * 5, [0, 1]), _unhold([1, 0, 0, 0, 0])]),
        # the row lets go first (nothing pushed), then the cache: pushed in the order of drop_ids
        "row_first": (*B0, [_TWO, _hold(5, 4, {}, [0, 1]), _unhold([1, 0, 0, 0, 0]), _unhold([0] * 5, [1, 0])]),
        # page 1 given up by row 0 and by the cache in one launch: pushed at the row's position, before page 3 of the drops
        "row_and_cache_together": (*B0, [_TWO, _hold(5, 4, {}, [3, 1]), _unhold([0, 1, 0, 0, 0]), _unhold([1, 0, 0, 0, 0], [3, 1])]),
        # a row maps two cached pages and the reserve grows it behind them (need 3, owned 2: one page popped)
        "hold_then_grow": (*B0, [_TWO, _hold(5, 4, {3: [0, 1]}), _reserve([1, 1, 1, 1, 1], 0, extra_rows=[0, 0, 0, 150, 0])]),
        # the scans cross a wave, the workgroup's stride; N = 700: more freed pages than the workgroup has threads
        "wave": (70, 4, 2, 150, _wide_ops(70, 150)),
        "stride": (300, 4, 2, 700, _wide_ops(300, 700)),
        # a chunk of the row loop exactly full; the largest batch the entries take: four chunks, the carry crosses three boundaries
        "chunk": (256, 4, 2, 600, _wide_ops(256, 600)),
        "full": (1024, 4, 2, 2400, _wide_ops(1024, 2400)),
        "many_freed": (300, 4, 2, 700, [_reserve(_i32([129] * 300), 1), _hold(300, 4, {}, range(698, -1, -7)),
                                        _unhold(_i32(np.ones(300)), range(5, 699, 7))]),
        # ---- broken invariants: the last op fails
        "take_negative": (*B0, [_TWO, _hold(5, 4, {2: [0]}) | dict(take=_i32([0, 0, -1, 0, 0]))]),
        "take_too_large": (*B0, [_TWO, _hold(5, 4, {2: [0, 1, 2, 3]}) | dict(take=_i32([0, 0, 5, 0, 0]))]),
        "hold_into_an_owner": (*B0, [_TWO, _hold(5, 4, {1: [0]})]),
        "hold_id_outside": (*B0, [_TWO, _hold(5, 4, {2: [0, 7]})]),
        "hold_id_negative": (*B0, [_TWO, _hold(5, 4, {2: [-1]})]),
        "hold_a_free_page": (*B0, [_TWO, _hold(5, 4, {2: [0, 5]})]),
        "cache_holds_a_free_page": (*B0, [_TWO, _hold(5, 4, {}, [4])]),
        "cache_hold_outside": (*B0, [_TWO, _hold(5, 4, {}, [0, 7])]),
        "hold_ids_twice": (*B0, [_TWO, _hold(5, 4, {}, [1, 0, 1])]),
        "more_given_up_than_held": (*B0, [_TWO, _unhold([1, 0, 0, 0, 0], [1])]),
        "drop_twice": (*B0, [_TWO, _hold(5, 4, {}, [2]), _unhold([0] * 5, [2, 2, 2])]),
        "drop_outside": (*B0, [_TWO, _unhold([0] * 5, [7])]),
        "unhold_bad_page_id": (*B0, [_TWO, _poke("page_ids", (1, 1), -3), _unhold([0, 1, 0, 0, 0])]),
        "unhold_bad_owned": (*B0, [_TWO, _poke("owned", 3, 5), _unhold([1, 0, 0, 0, 0])]),
        "unhold_bad_count": (*B0, [_TWO, _poke("count", None, 8), _unhold([1, 0, 0, 0, 0])]),
        "count_above_n": (*B0, [_TWO, _poke("count", None, 6), _unhold([1, 0, 0, 0, 0])]),
        "popped_page_has_holders": (*B0, [_TWO, _poke("refs", 4, 1), _reserve([1, 1, 10, 1, 1], 1)]),
    }


BROKEN = ("take_negative", "take_too_large", "hold_into_an_owner", "hold_id_outside", "hold_id_negative", "hold_a_free_page",
          "cache_holds_a_free_page", "cache_hold_outside", "hold_ids_twice", "more_given_up_than_held", "drop_twice", "drop_outside",
          "unhold_bad_page_id", "unhold_bad_owned", "unhold_bad_count", "count_above_n", "popped_page_has_holders")
