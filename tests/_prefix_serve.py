"""The setting of tests/test_prefix_serve_gpu.py and a host-only simulation of DecodeEngine.serve under a prefix cache: the real
`serving.Scheduler` and `prefix.PrefixCache` over the loop restatement of the counted pool (tests/_page_ref_cases.py) and texts whose
lengths are known in advance - length limits only, no stop sequence, so a row emits one token per round until its limit or until the
pool refuses it.  What the model would generate is unknown here and does not matter: generated tokens are stand-ins that no prompt
holds, so the only hits are those of the common prefix and of a resumed request's own text - which is what the GPU run must show too.

A dozen requests share a prefix of 128 tokens and go on with 5 .. 60 tokens of their own; B = 4 rows over a pool of N pages."""
import random

import numpy as np

import _page_ref_cases as R
from qserve_amd.prefix import PrefixCache
from qserve_amd.serving import Scheduler

B, CAP_P, MAX_NEW, N, POLL, CHUNK = 4, 256, 80, 10, 4, 128
LIVE, LENGTH, NO_PAGES = 0, 2, 3
OWN = [(20, 70), (60, 40), (5, 75), (33, 50), (50, 12), (12, 30), (41, 66), (7, 9), (58, 25), (26, 44), (64, 20), (18, 60)]   # (own tokens, max_new)


def requests():
    r = random.Random(23)
    prefix = [r.randrange(512) for _ in range(128)]
    return [(prefix + [r.randrange(512) for _ in range(own)], new) for own, new in OWN]


def simulate(reqs, prefix_cache=True, batch=B, max_len=CAP_P + MAX_NEW, pages=N, poll=POLL):
    """-> (per request dict(length, reason, preempted_at, hit_tokens), stats) as serve() must report them."""
    mb = (max_len + 63) // 64 + 1
    cache = PrefixCache() if prefix_cache else None
    sched = Scheduler(reqs, batch, max_len, NO_PAGES, pool_pages=pages, advance=1, prefix=cache)
    st = R.new_state(batch, mb, 1, pages)
    lengths, finished, limits = np.ones(batch, np.int32), np.full(batch, LENGTH, np.int32), np.zeros(batch, np.int32)
    texts, row_cached = [[0] for _ in range(batch)], {}

    def release(rows, drops=()):
        nonlocal st
        for b in rows:
            if cache is not None:
                cache.row_released(row_cached.pop(b, ()))
        st = R.unhold_loop(st, np.isin(np.arange(batch), rows).astype(np.int32), list(drops))
        assert st["error"] == 0

    def hold(rows, ids=()):
        nonlocal st
        st = R.hold_loop(st, *(R._hold(batch, mb, rows, ids)[k] for k in ("take", "src", "hold_ids")))
        assert st["error"] == 0

    while True:
        ended, starved = sched.ended()
        kept = []
        if cache is not None:
            for b in starved:
                n = (sched.lens[b] - 1) // 64
                fresh = cache.insert(texts[b][:sched.lens[b] - 1], st["page_ids"][b, :n].tolist())
                row_cached[b] = list(row_cached.get(b, ())) + fresh
                kept += fresh
            sched.stats["inserted_pages"] += len(kept)
            if kept:
                hold({}, kept)
        sched.retire([texts[b] + [0] * (max_len - len(texts[b])) for b in starved],
                     {b: len(row_cached.get(b, ())) for b in ended} if cache is not None else None)
        if ended:
            for b in ended:
                lengths[b], limits[b], finished[b], texts[b] = 1, 0, LENGTH, [0]
            release(ended)
        rows, batch_reqs, *evict = sched.place()
        if evict and evict[0][0]:
            release([], cache.evict(*evict[0]))
        if rows:
            before = len(cache) if cache is not None else 0
            cached = [cache.match(q["prompt"], len(q["prompt"]) - 1) if cache is not None else [] for q in batch_reqs]
            for b, q in zip(rows, batch_reqs):
                finished[b], limits[b] = LIVE, q["start"] + q["max_new"]
            release(rows)
            if any(cached):
                hold({b: ids for b, ids in zip(rows, cached) if ids})
            extra = np.zeros(batch, np.int32)
            extra[rows] = [len(q["prompt"]) for q in batch_reqs]
            st, finished = R.reserve_loop(st, np.ones(batch, np.int32), 0, extra, finished)
            new = []
            for b, q, ids in zip(rows, batch_reqs, cached):
                P = len(q["prompt"])
                if cache is not None:
                    row_ids = st["page_ids"][b, :P // 64].tolist()
                    fresh = cache.insert(q["prompt"], row_ids) if min(row_ids, default=0) >= 0 else []
                    row_cached[b] = ids + fresh
                    new += fresh
                # the first token: a stand-in no prompt holds (request, position)
                texts[b], lengths[b] = list(q["prompt"]) + [-(1 + q["i"] * 100000 + P)], P + 1
                if finished[b] == LIVE and lengths[b] >= limits[b]:
                    finished[b] = LENGTH
            if new:
                hold({}, new)
            if cache is not None:
                sched.stats["inserted_pages"] += len(cache) - before
        if sched.idle():
            break
        for _ in range(poll):
            st, finished = R.reserve_loop(st, lengths, 1, None, finished)
            assert st["error"] == 0
            for b in range(batch):
                if finished[b] == LIVE:
                    lengths[b] += 1
                    texts[b].append(-(1 + sched.slots[b]["i"] * 100000 + int(lengths[b]) - 1))
                    if lengths[b] >= limits[b]:
                        finished[b] = LENGTH
        sched.observe(poll, finished.tolist(), lengths.tolist(), st["count"], st["owned"].tolist())
    if cache is not None:
        R.check_invariant(st, cache.by_page)
    out, stats = sched.output([[0] * max_len for _ in reqs])
    return [dict(length=r["length"], reason=r["reason"], preempted_at=o["preempted_at"], hit_tokens=o.get("hit_tokens"))
            for r, o in zip(sched.results, out)], stats, (st, cache)
