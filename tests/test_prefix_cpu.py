"""qserve_amd.prefix.PrefixCache and serving.Scheduler(prefix=...) on the host alone: chains of whole pages, the limit that keeps a
prompt's last token out, salts, what insert enters and what it must leave out, leaf-first least-recently-used eviction, `keep`,
`evictable()` never promising a page `evict` cannot deliver, row holders - and the scheduler's charge, eviction request and the
re-placement of a preempted request, driven with hand-written observations as tests/test_serving_cpu.py does."""
import random

import pytest

from qserve_amd.prefix import PrefixCache
from qserve_amd.serving import Scheduler


def _toks(seed, n):
    r = random.Random(seed)
    return [r.randrange(512) for _ in range(n)]


X = _toks(1, 200)


def test_a_chain_is_matched_page_by_page_and_the_limit_keeps_the_last_token_out():
    c = PrefixCache()
    assert c.insert(X[:150], [10, 11, 12]) == [10, 11] and len(c) == 2      # two whole pages; the third id is not needed
    assert c.peek(X[:150], 149) == [10, 11] and c.peek(X, 200) == [10, 11]
    assert c.peek(X[:128], 127) == [10]                                     # exactly 128 tokens: limit P - 1 = 127 cuts at one page
    assert c.peek(X[:128], 128) == [10, 11] and c.peek(X[:64], 63) == [] and c.peek(X[:65], 64) == [10]
    assert c.peek(X[:100], 1000) == [10]                                    # never beyond the tokens themselves
    other = X[:64] + _toks(2, 100)
    assert c.peek(other, 163) == [10]                                       # the chain ends where the tokens part
    assert c.peek(_toks(3, 64) + X[64:], 199) == []                         # a page is keyed by its parent: no match in the middle
    assert c.insert(other, [10, 13]) == [13] and c.peek(other, 163) == [10, 13] and c.peek(X, 199) == [10, 11]


def test_salts_separate_chains():
    c = PrefixCache()
    assert c.insert(X[:128], [0, 1], salt=7) == [0, 1]
    assert c.peek(X[:150], 149) == [] and c.match(X[:150], 149, salt=8) == [] and c.peek(X[:150], 149, salt=7) == [0, 1]
    assert c.insert(X[:128], [2, 3]) == [2, 3] and c.peek(X[:150], 149) == [2, 3]


def test_insert_leaves_out_what_is_cached_under_another_id_and_everything_behind_it():
    c = PrefixCache()
    assert c.insert(X[:192], [0, 1, 2]) == [0, 1, 2]
    # a row that matched one page and recomputed the rest under its own ids: position 1 is cached under 1, not 8 - 8 and 9 stay private
    assert c.insert(X[:192], [0, 8, 9]) == [] and c.peek(X, 199) == [0, 1, 2] and len(c) == 3
    # a longer text of a row that holds the cached ids extends the chain
    assert c.insert(X[:200] + _toks(5, 56), [0, 1, 2, 5]) == [5] and len(c) == 4
    # an id the cache already has elsewhere is never entered twice
    assert c.insert(_toks(6, 128), [7, 1]) == [7] and len(c) == 5


def test_row_holders_are_counted():
    c = PrefixCache()
    new = c.insert(X[:128], [0, 1])                                         # the inserting row holds both
    assert c.evictable() == 0 and c.evict(5) == []
    assert c.match(X[:150], 149) == [0, 1] and c.match(X[:100], 99) == [0]  # holders: page 0: 3, page 1: 2
    c.row_released(new)
    c.row_released([0, 1, 44])                                              # (44: a private page of that row)
    assert c.evictable() == 1 and c.peek(X[:150], 149) == [0, 1]            # page 1 has no holder left, page 0 has the third row
    c.row_released([0])
    assert c.evictable() == 2
    with pytest.raises(AssertionError, match="no row holder"):
        c.row_released([0])


def test_eviction_is_leaf_first_and_least_recently_used():
    c = PrefixCache()
    a, b = X[:64] + _toks(10, 64), X[:64] + _toks(11, 64)
    c.row_released(c.insert(a + _toks(12, 64), [0, 1, 2]))                  # 0 - 1 - 2
    c.row_released(c.insert(b, [0, 3]))                                     # 0 - 3
    assert c.evictable() == 4
    c.row_released(c.match(a, 1000))                                        # 0 and 1 are used again; of the leaves 2 is older than 3
    assert c.evict(1) == [2]                                                # ... which exposes 1, used after 3
    assert c.evict(2) == [3, 1]
    assert c.evictable() == 1 and c.evict(9) == [0] and len(c) == 0 and c.evict(1) == []


def test_keep_spares_ids_and_evictable_promises_only_what_evict_delivers():
    c = PrefixCache()
    c.row_released(c.insert(X[:192], [0, 1, 2]))
    c.row_released(c.insert(_toks(20, 128), [5, 6]))
    assert c.evictable() == 5 and c.evictable(keep=[1]) == 3                # 1 is kept, 0 lies above it: 2, 5, 6 remain
    assert sorted(c.evict(9, keep=[1])) == [2, 5, 6] and c.peek(X, 199) == [0, 1]
    held = c.match(X[:100], 99)                                             # a row holds page 0: page 1 below it can still go
    assert held == [0] and c.evictable() == 1 and c.evict(9) == [1] and c.evictable() == 0
    c.row_released(held)
    r = random.Random(0)
    for trial in range(50):                                                 # random trees, holders and keeps: the promise is exact
        c = PrefixCache()
        texts, nxt = [], 0
        for _ in range(6):
            base = r.choice(texts)[:64 * r.randrange(0, 3)] if texts else []
            t = base + _toks(r.randrange(10 ** 6), 64 * r.randrange(1, 4))
            ids = c.peek(t, len(t))
            ids += list(range(nxt, nxt + len(t) // 64 - len(ids)))
            nxt += len(t) // 64
            new = c.insert(t, ids)
            if r.random() < 0.7:
                c.row_released(new)
            texts.append(t)
        keep = [i for i in range(nxt) if r.random() < 0.2]
        n = c.evictable(keep)
        assert len(c.evict(10 ** 6, keep)) == n and c.evictable(keep) == 0


# ---- the scheduler -----------------------------------------------------------------------------------------------------------------
STARVED = 3


def test_hits_reduce_the_charge_and_eviction_is_asked_for_only_when_free_pages_do_not_cover():
    c = PrefixCache()
    c.row_released(c.insert(X[:128], [0, 1]))                               # two cached pages nobody holds
    c.row_released(c.insert(_toks(30, 64), [2]))                            # and a third, older by use below
    c.row_released(c.match(X[:128], 1000))
    reqs = [(X[:150], 10), (X[:128] + _toks(31, 30), 10), (_toks(32, 100), 5)]
    s = Scheduler(reqs, 3, 400, STARVED, pool_pages=8, prefix=c)
    s.free = 5                                                              # 8 pages: 3 cached, 5 free
    rows, batch, (evict, keep) = s.place()
    # charges: ceil(151 / 64) - 2 = 1, ceil(159 / 64) - 2 = 1, ceil(101 / 64) - 0 = 2
    assert rows == [0, 1, 2] and evict == 0 and sorted(keep) == [0, 0, 1, 1] and s.free == 1
    assert s.stats["hit_tokens"] == 256 and s.stats["evicted"] == 0 and [q["hit_tokens"] for q in batch] == [[128], [128], [0]]
    assert len(c) == 3 and c.evictable() == 3                               # the scheduler only peeks

    s = Scheduler(reqs, 3, 400, STARVED, pool_pages=8, prefix=c)
    s.free = 3                                                              # 4 wanted, 3 free: one eviction, and never a peeked page
    rows, batch, (evict, keep) = s.place()
    assert rows == [0, 1, 2] and evict == 1 and s.free == 0 and s.stats["evicted"] == 1
    assert c.evict(evict, keep) == [2]

    s = Scheduler(reqs, 3, 400, STARVED, pool_pages=8, prefix=c)
    s.free = 1                                                              # after that eviction nothing else can go: the third blocks
    rows, batch, (evict, keep) = s.place()
    assert rows == [0] and evict == 0 and s.free == 0 and len(s.queue) == 2
    rows, batch, (evict, keep) = s.place()
    assert rows == [] and evict == 0


def test_without_a_prefix_cache_place_returns_what_it_always_did():
    s = Scheduler([(X[:10], 3)], 2, 100, STARVED, pool_pages=4)
    assert s.place() == ([0], [s.slots[0]]) and "hit_tokens" not in s.stats and "hit_tokens" not in s.slots[0]
    with pytest.raises(AssertionError, match="shares the pages of a pool"):
        Scheduler([(X[:10], 3)], 2, 100, STARVED, prefix=PrefixCache())
    with pytest.raises(AssertionError, match="can never fit the pool"):
        Scheduler([(X[:150], 60)], 2, 400, STARVED, pool_pages=3, prefix=PrefixCache())


def test_a_preempted_request_with_its_pages_still_cached_is_charged_only_the_remainder():
    c = PrefixCache()
    s = Scheduler([(X[:100], 80)], 2, 400, STARVED, pool_pages=4, prefix=c)
    rows, batch, (evict, keep) = s.place()
    assert rows == [0] and evict == 0 and s.free == 2                       # ceil(101 / 64) = 2 pages, nothing cached
    held = c.insert(X[:100], [0, 1])                                        # what admit enters: the one whole page
    assert held == [0]
    # the row grew to 150 tokens over pages 0, 1, 2, wanted a fourth page another row took, and starved
    s.observe(8, [STARVED, 0], [150, 1], free=0, owned=[3, 0])
    ended, starved = s.ended()
    assert ended == starved == [0]
    text = X[:150]
    held += c.insert(text[:149], [0, 1, 2])                                 # serve: the whole pages of text[:L - 1] before the release
    assert held == [0, 1]
    s.retire([text + [0] * 250], cached={0: 2})
    c.row_released(held)
    assert s.free == 1 and s.stats["preempted"] == 1 and s.queue[0]["prompt"] == text and s.queue[0]["preempted_at"] == [50]
    rows, batch, (evict, keep) = s.place()
    # P = 150: ceil(151 / 64) = 3 pages, 2 of them cached: one page charged, no eviction, the peeked pages spared
    assert rows == [0] and evict == 0 and sorted(keep) == [0, 1] and s.free == 0
    assert batch[0]["hit_tokens"] == [0, 128] and s.stats["hit_tokens"] == 128 and s.stats["admitted"] == 2
