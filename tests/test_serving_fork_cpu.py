"""`qserve_amd.serving.Scheduler` with requests of n samples, on hand-written observations: no engine, no device.  Every expected value
is derived by hand from the rules in its docstrings (pages of 64 slots; a leader needs ceil((P + 1) / 64) of them, a follower one)."""
import pytest

import test_serving_cpu as T
from qserve_amd.serving import Scheduler

NO_PAGES, STOPPED, LENGTH = T.NO_PAGES, T.STOPPED, T.LENGTH


def _sched(reqs, batch, pool, max_new=4, max_len=300, **kw):
    return Scheduler([([7] * p, max_new, n) for p, n in reqs], batch, max_len, NO_PAGES, pool_pages=pool, **kw)


@pytest.mark.parametrize("name", [n for n in dir(T) if n.startswith("test_") and n != "test_the_finished_codes_are_those_of_the_stop_rule"])
def test_n_equal_one_is_the_scheduler_as_it_was(monkeypatch, name):
    """Every expectation of tests/test_serving_cpu.py holds when each of its requests says n = 1."""
    monkeypatch.setattr(T, "Scheduler", lambda reqs, *a, **kw: Scheduler([(p, m, 1) for p, m in reqs], *a, **kw))
    fn = getattr(T, name)
    for args in getattr(fn, "pytestmark", [None])[0].args[1] if hasattr(fn, "pytestmark") else [()]:
        fn(*args)


def test_two_tuples_and_n_equal_one_leave_the_same_state():
    a = Scheduler([([7] * 70, 4), ([7] * 5, 4)], 2, 200, NO_PAGES, pool_pages=6)
    b = Scheduler([([7] * 70, 4, 1), ([7] * 5, 4, 1)], 2, 200, NO_PAGES, pool_pages=6)
    for s in (a, b):
        s.place()
        s.observe(4, [LENGTH, 0], [74, 9], free=3, owned=[2, 1])
        s.retire()
    assert a.__dict__ == b.__dict__ and "forked" not in a.stats and a.copy_rows == {} and a.forks == {}
    assert a.reqs[0] == dict(i=0, prompt=[7] * 70, start=70, max_new=4, preempted_at=[])


def test_a_group_is_placed_when_n_rows_are_free_and_blocks_the_queue_until_then():
    s = _sched([(5, 1), (70, 3), (5, 1)], batch=4, pool=9)
    rows, reqs = s.place()
    # request 0 in row 0; the group's leader in row 1, its followers in rows 2 and 3; request 2 waits for a row
    assert rows == [0, 1] and [q["i"] for q in reqs] == [0, 1] and s.copy_rows == {1: [2, 3]}
    assert [s.slots[b]["i"] for b in range(4)] == [0, 1, 2, 3] and [s.slots[b]["k"] for b in (1, 2, 3)] == [0, 1, 2]
    assert s.free == 9 - 1 - (2 + 2) and s.stats["admitted"] == 4 and s.stats["forked"] == 2      # the leader's 2 pages, 1 per follower
    assert [q["i"] for q in s.queue] == [4] and "copies" not in s.slots[1]
    # fewer than n rows free: the group waits, and what is behind it with it
    s = _sched([(5, 1), (5, 1), (70, 3), (5, 1)], batch=4, pool=9)
    rows, reqs = s.place()
    assert rows == [0, 1] and s.copy_rows == {} and s.slots[2:] == [None, None] and [q["i"] for q in s.queue] == [2, 5]
    s.observe(4, [STOPPED, 0, LENGTH, LENGTH], [9, 9, 1, 1], free=7, owned=[1, 1, 0, 0])
    s.retire()
    rows, reqs = s.place()                                                  # rows 0, 2, 3 are free now: leader in 0
    assert rows == [0] and s.copy_rows == {0: [2, 3]} and s.free == 8 - 4 and [q["i"] for q in s.queue] == [5]
    # pages: the leader's ceil(71 / 64) = 2 and one per follower must be free at once
    s = _sched([(70, 3)], batch=4, pool=4)
    s.free = 3
    assert s.place() == ([], []) and s.copy_rows == {}
    s.free = 4
    assert s.place()[0] == [0] and s.free == 0


def test_a_member_is_credited_the_shared_pages_only_when_the_last_sibling_retires():
    s = _sched([(150, 3)], batch=3, pool=12, max_new=40)                   # P = 150: 2 whole pages shared, a tail page each
    assert s.place()[0] == [0] and s.copy_rows == {0: [1, 2]} and s.free == 12 - 3 - 2
    s.observe(8, [0, STOPPED, 0], [160, 158, 160], free=7, owned=[3, 3, 3])
    assert s.retire() == [(1, 1)] and s.free == 7 + 1                       # row 1's own page; the truth is 8
    s.observe(8, [LENGTH, LENGTH, 0], [190, 1, 168], free=8, owned=[3, 0, 3])
    assert s.retire() == [(0, 0)] and s.free == 8 + 1                       # row 2 still holds the two shared pages
    s.observe(8, [LENGTH, LENGTH, STOPPED], [1, 1, 200], free=8, owned=[0, 0, 4])
    assert s.retire() == [(2, 2)] and s.free == 12 and s.forks == {}        # the last one: all 4 of its pages
    assert s.idle()


def test_a_preempted_sample_resumes_alone_with_its_text():
    s = _sched([(150, 3), (5, 1)], batch=3, pool=6, max_new=60)
    assert s.place()[0] == [0] and s.free == 1
    s.observe(8, [0, 0, NO_PAGES], [193, 193, 192], free=0, owned=[4, 3, 3])   # rows 0 and 1 took the last pages
    text = list(range(300))
    assert s.retire([text]) == [] and s.stats["preempted"] == 1
    q = s.queue[0]
    assert [x["i"] for x in s.queue] == [2, 3] and q["prompt"] == text[:192] and q["preempted_at"] == [42] and q["k"] == 2
    assert s.free == 0 + 1 and s.forks.keys() == {0, 1}                    # its tail page alone: the siblings hold the shared two
    assert s.place() == ([], [])                                            # 193 slots need 4 pages: it waits, request 1 behind it
    s.observe(8, [LENGTH, STOPPED, LENGTH], [210, 200, 1], free=0, owned=[4, 4, 0])
    assert s.retire() == [(0, 0), (1, 1)] and s.free == 2 + 4              # row 0: 4 - 2 shared, row 1 the last: all 4
    rows, reqs = s.place()
    assert rows == [0, 1] and [q["i"] for q in reqs] == [2, 3] and s.copy_rows == {} and 0 not in s.forks   # alone, like any request
    s.observe(8, [LENGTH, LENGTH, LENGTH], [210, 9, 1], free=1, owned=[4, 1, 0])
    s.retire()
    assert s.idle()
    texts = [[k] * 300 for k in range(4)]
    out, stats = s.output(texts)
    assert out == [dict(tokens=[0] * 60, reason=LENGTH, preempted_at=[],
                        samples=[dict(tokens=[0] * 60, reason=LENGTH, preempted_at=[]), dict(tokens=[1] * 50, reason=STOPPED, preempted_at=[]),
                                 dict(tokens=[2] * 60, reason=LENGTH, preempted_at=[42])]),
                   dict(tokens=[3] * 4, reason=LENGTH, preempted_at=[])]
    assert stats == dict(rounds=24, read_backs=5, admitted=5, preempted=1, peak_pages=6, forked=2)


def test_with_a_prefix_cache_the_leader_is_charged_what_it_cannot_map():
    from qserve_amd.prefix import PrefixCache
    cache = PrefixCache()
    prompt = list(range(150))
    assert cache.insert(prompt, [0, 1]) == [0, 1]
    cache.row_released([0, 1])
    s = Scheduler([(prompt, 4, 3)], 3, 300, NO_PAGES, pool_pages=6, prefix=cache)
    s.free = 3                                                              # (the cache holds pages 0 and 1; one more is in use)
    rows, reqs, (evict, keep) = s.place()
    # 3 pages for the prompt, 2 of them mapped, + 2 followers: 3 free pages cover it, nothing is evicted
    assert rows == [0] and s.copy_rows == {0: [1, 2]} and (evict, keep) == (0, [0, 1]) and s.free == 0
    assert reqs[0]["hit_tokens"] == [128] and s.stats["forked"] == 2
    s.observe(4, [LENGTH, LENGTH, LENGTH], [154, 154, 154], free=0, owned=[3, 3, 3])
    s.retire(cached={0: 2, 1: 2, 2: 2})
    assert s.free == 3                                                      # one tail page each: the cached pages stay cached
    out, stats = s.output([list(range(300))] * 3)
    assert out[0]["hit_tokens"] == [128] and len(out[0]["samples"]) == 3 and "hit_tokens" not in out[0]["samples"][0]


@pytest.mark.parametrize("match, reqs, kw", [
    (r"request 1 asks for n=4 samples - 1 .. batch = 3", [([1] * 5, 3), ([1] * 5, 3, 4)], dict(pool_pages=9)),
    (r"request 0 asks for n=0 samples", [([1] * 5, 3, 0)], dict(pool_pages=9)),
    (r"request 0 can never fit the pool: its prompt of 70 tokens and 2 further samples need 4 pages at once, the pool has 3",
     [([1] * 70, 3, 3)], dict(pool_pages=3)),
    (r"request 0 can never fit the pool: prompt 70 \+ max_new_tokens 60 need 3 pages", [([1] * 70, 60, 2)], dict(pool_pages=2)),
    (r"request 0 asks for n=2 samples - they share the pages of a page pool", [([1] * 5, 3, 2)], {}),
    (r"request 0 - \(prompt_tokens, max_new_tokens\) or", [([1] * 5, 3, 2, 2)], dict(pool_pages=9)),
])
def test_a_group_that_can_never_fit_is_refused_before_any_state_exists(match, reqs, kw):
    with pytest.raises(AssertionError, match=match):
        Scheduler(reqs, 3, 200, NO_PAGES, **kw)
