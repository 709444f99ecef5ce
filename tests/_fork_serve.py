"""The setting of tests/test_fork_serve_gpu.py and a host-only simulation of DecodeEngine.serve with requests of n samples: the real
`serving.Scheduler` over the loop restatements of the counted pool and of the fork (tests/_page_fork_cases.py) and texts whose lengths
are known in advance - length limits only, no stop sequence, so a row emits one token per round until its limit or until the pool
refuses it (the simulation of tests/_prefix_serve.py, without a cache and with forks).

Six requests of 130 .. 190 prompt tokens (two whole pages each) ask for 3 samples of 20 .. 60 tokens; B = 6 rows."""
import random

import numpy as np

import _page_fork_cases as K

B, CAP_P, MAX_NEW, POLL, CHUNK = 6, 200, 64, 4, 128
N_SMALL, N_LARGE = 11, 40                                                # a pool that preempts (found with `simulate`), one that never does
LIVE, LENGTH, NO_PAGES = 0, 2, 3
SHAPES = [(150, 40), (133, 60), (190, 20), (141, 55), (170, 33), (129, 48)]     # (prompt tokens, max_new)


def requests(n=3):
    r = random.Random(31)
    prompts = [([r.randrange(512) for _ in range(p)], new) for p, new in SHAPES]
    return [(p, new, n) for p, new in prompts] if n > 1 else [(p, new) for p, new in prompts for _ in range(3)]


def simulate(reqs, pages, batch=B, max_len=CAP_P + MAX_NEW, poll=POLL):
    """-> (per sample of `Scheduler.reqs` dict(length, reason, preempted_at), stats, the pool's last state)."""
    from qserve_amd.serving import Scheduler
    mb = (max_len + 63) // 64 + 1
    sched = Scheduler(reqs, batch, max_len, NO_PAGES, pool_pages=pages, advance=1)
    st = K.new_state(batch, mb, 1, pages, page_bytes=1)
    lengths, finished, limits = np.ones(batch, np.int32), np.full(batch, LENGTH, np.int32), np.zeros(batch, np.int32)
    while True:
        ended, starved = sched.ended()
        sched.retire([[0] * max_len for _ in starved])
        if ended:
            for b in ended:
                lengths[b], limits[b], finished[b] = 1, 0, LENGTH
            st = K.R.unhold_loop(st, np.isin(np.arange(batch), ended).astype(np.int32), [])
        rows, batch_reqs = sched.place()
        if rows:
            every = rows + [r for b in rows for r in sched.copy_rows.get(b, [])]
            for b in every:
                finished[b], limits[b] = LIVE, sched.slots[b]["start"] + sched.slots[b]["max_new"]
            st = K.R.unhold_loop(st, np.isin(np.arange(batch), every).astype(np.int32), [])
            extra = np.zeros(batch, np.int32)
            extra[rows] = [len(q["prompt"]) for q in batch_reqs]
            st, finished = K.R.reserve_loop(st, np.ones(batch, np.int32), 0, extra, finished)
            if sched.copy_rows:
                told = np.ones(batch, np.int32)
                told[rows] = [len(q["prompt"]) + 1 for q in batch_reqs]
                st, finished = K.fork_loop(st, K._fork(batch, {r: b for b in rows for r in sched.copy_rows.get(b, [])}, told)["src_rows"], told,
                                           finished)
            for b in every:
                lengths[b] = len(sched.slots[b]["prompt"]) + 1
                if finished[b] == LIVE and lengths[b] >= limits[b]:
                    finished[b] = LENGTH
        assert st["error"] == 0 and sched.free <= st["count"]              # the estimate is never above the truth
        if sched.idle():
            break
        for _ in range(poll):
            st, finished = K.R.reserve_loop(st, lengths, 1, None, finished)
            for b in range(batch):
                if finished[b] == LIVE:
                    lengths[b] += 1
                    if lengths[b] >= limits[b]:
                        finished[b] = LENGTH
        sched.observe(poll, finished.tolist(), lengths.tolist(), st["count"], st["owned"].tolist())
    K.check_invariant(st)
    sched.output([[0] * max_len for _ in sched.reqs])                       # (the read-back of the texts counts in stats)
    return [dict(length=r["length"], reason=r["reason"], preempted_at=q["preempted_at"]) for r, q in zip(sched.results, sched.reqs)], sched.stats, st
