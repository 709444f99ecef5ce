"""`qserve_amd.serving.Scheduler`, the policy of DecodeEngine.serve, on hand-written observations: no engine, no device, no
stand-in for the library (one test alone looks at the library's module, for the `finished` codes restated here).  Every expected value below is derived by hand from the rules in its docstrings (pages of 64 slots; a placement needs
ceil((P + 1) / 64) of them)."""
import pytest

from qserve_amd.serving import Scheduler

NO_PAGES, STOPPED, LENGTH = 3, 1, 2                                      # the `finished` codes of qserve_amd.stopping


def _sched(prompts, batch, pool, max_new=4, max_len=200, **kw):
    return Scheduler([([7] * p, max_new) for p in prompts], batch, max_len, NO_PAGES, pool_pages=pool, **kw)


def test_the_finished_codes_are_those_of_the_stop_rule(built_lib):
    from qserve_amd import stopping
    assert (NO_PAGES, STOPPED, LENGTH) == (stopping.NO_PAGES, stopping.STOPPED, stopping.LENGTH)


def test_the_first_request_that_does_not_fit_blocks_the_queue():
    s = _sched([5, 130, 5], batch=2, pool=3)                             # they need 1, 3 and 1 pages
    rows, reqs = s.place()
    assert rows == [0] and [q["i"] for q in reqs] == [0] and s.free == 2
    assert s.slots[1] is None and [q["i"] for q in s.queue] == [1, 2]    # row 1 is free and request 2 would fit: it waits all the same
    assert s.place() == ([], []) and s.stats["admitted"] == 1 and not s.idle()


def test_with_one_more_page_the_second_is_placed_and_the_third_waits_for_a_row():
    s = _sched([5, 130, 5], batch=2, pool=4)
    rows, reqs = s.place()
    assert rows == [0, 1] and [q["i"] for q in reqs] == [0, 1] and s.free == 0
    assert [q["i"] for q in s.queue] == [2] and s.stats["admitted"] == 2


def test_starved_rows_return_to_the_front_in_row_order_with_their_text():
    s = _sched([60, 100, 5], batch=2, pool=4, max_new=90)
    assert s.place()[0] == [0, 1] and [q["i"] for q in s.queue] == [2]
    lengths = [70, 128]
    s.observe(8, [NO_PAGES, NO_PAGES], lengths, free=0, owned=[2, 2])
    assert s.ended() == ([0, 1], [0, 1])
    texts = [list(range(1000, 1200)), list(range(2000, 2200))]
    assert s.retire(texts) == []                                         # nobody is done
    assert [q["i"] for q in s.queue] == [0, 1, 2] and s.slots == [None, None]
    for b, q in enumerate(list(s.queue)[:2]):
        assert q["prompt"] == texts[b][:lengths[b]] and q["start"] == [60, 100][b] and q["max_new"] == 90
        assert q["preempted_at"] == [lengths[b] - q["start"]]
    assert s.free == 4 and s.owned == [0, 0] and s.results == [None] * 3
    assert s.stats["preempted"] == 2 and s.stats["read_backs"] == 2      # the burst's, and the texts'
    # the re-admission needs ceil((lengths[b] + 1) / 64) pages: 2 for 71 slots, 3 for 129 - which the 2 pages left do not cover
    rows, reqs = s.place()
    assert rows == [0] and reqs[0]["i"] == 0 and s.free == 2 and [q["i"] for q in s.queue] == [1, 2]


def test_retiring_gives_the_pages_back_and_the_peak_is_taken_at_the_observations():
    s = _sched([5, 70], batch=2, pool=6, max_new=90)
    s.place()
    assert s.free == 3                                                   # the estimate: 1 and 2 pages taken
    s.observe(8, [0, 0], [13, 78], free=3, owned=[1, 2])
    assert s.ended() == ([], []) and s.retire() == [] and s.stats["peak_pages"] == 3
    s.observe(8, [0, STOPPED], [64, 130], free=1, owned=[2, 3])
    assert s.stats["peak_pages"] == 5 and s.ended() == ([1], [])
    assert s.retire() == [(1, 1)] and s.results[1] == dict(length=130, reason=STOPPED)
    assert s.free == 4 and s.owned == [2, 0] and s.slots[1] is None and s.slots[0]["i"] == 0
    s.observe(8, [LENGTH, LENGTH], [95, 1], free=4, owned=[2, 0])        # row 1 is empty: what it shows ends nobody
    assert s.ended() == ([0], []) and s.retire() == [(0, 0)] and s.free == 6 and s.stats["peak_pages"] == 5
    assert s.stats == dict(rounds=24, read_backs=3, admitted=2, preempted=0, peak_pages=5)


def test_without_a_pool_nothing_is_accounted():
    s = Scheduler([([7] * 130, 4)] * 3, 2, 200, NO_PAGES, static_pages=10)
    assert s.place()[0] == [0, 1] and s.free is None and s.stats["peak_pages"] == 10
    s.observe(1, [LENGTH, 0], [134, 131])
    assert s.retire() == [(0, 0)] and s.place()[0] == [0] and s.free is None and s.stats["peak_pages"] == 10


@pytest.mark.parametrize("match, reqs, kw", [
    ("request 0 - a prompt of at least one token and max_new_tokens >= 1", [([], 3)], {}),
    ("request 1 - a prompt of at least one token", [([1], 3), ([1], 0)], {}),
    (r"request 0 can never fit max_len: prompt 60 \+ max_new_tokens 41 > 100", [([1] * 60, 41)], {}),
    (r"request 1 can never fit the pool: prompt 90 \+ max_new_tokens 10 need 2 pages, the pool has 1", [([1] * 5, 3), ([1] * 90, 10)], {}),
    (r"request 0 can never fit the pool: prompt 60 \+ max_new_tokens 4 need 2 pages", [([1] * 60, 4)], dict(advance=2)),
])
def test_a_request_that_can_never_fit_is_refused_before_any_state_exists(match, reqs, kw):
    with pytest.raises(AssertionError, match=match):
        Scheduler(reqs, 3, 100, NO_PAGES, pool_pages=1, **kw)
    assert Scheduler([([1] * 60, 4)], 3, 100, NO_PAGES, pool_pages=1).place()[0] == [0]      # 63 slots + the round's 1: one page


def test_a_whole_run_ends_idle_and_counts_every_admission():
    """Three requests through two rows and 3 pages, one preemption: every observation is what a pool would show for the lengths."""
    s = _sched([5, 100, 5], batch=2, pool=3, max_new=40)
    assert s.place()[0] == [0, 1] and s.free == 0 and not s.idle()       # 1 + 2 pages: the pool is full; request 2 waits for a row
    s.observe(8, [0, NO_PAGES], [13, 128], free=0, owned=[1, 2])         # row 1 wanted its third page
    assert s.ended() == ([1], [1]) and s.retire([[9] * 200]) == []
    assert [q["i"] for q in s.queue] == [1, 2] and s.free == 2
    assert s.place() == ([], []) and not s.idle()                        # 129 slots need 3 pages: request 1 blocks request 2
    s.observe(8, [STOPPED, LENGTH], [20, 1], free=2, owned=[1, 0])
    assert s.retire() == [(0, 0)] and s.free == 3
    assert s.place()[0] == [0] and s.slots[0]["i"] == 1 and s.free == 0 and not s.idle()
    s.observe(8, [LENGTH, LENGTH], [140, 1], free=0, owned=[3, 0])
    assert s.retire() == [(0, 1)]
    assert s.place()[0] == [0] and s.slots[0]["i"] == 2 and not s.idle()
    s.observe(3, [STOPPED, LENGTH], [9, 1], free=2, owned=[1, 0])
    assert s.retire() == [(0, 2)] and s.place() == ([], []) and s.idle()
    out, stats = s.output([[0] * 5 + [1] * 195, [0] * 100 + [2] * 100, [0] * 5 + [3] * 195])
    assert out == [dict(tokens=[1] * 15, reason=STOPPED, preempted_at=[]), dict(tokens=[2] * 40, reason=LENGTH, preempted_at=[28]),
                   dict(tokens=[3] * 4, reason=STOPPED, preempted_at=[])]
    assert stats == dict(rounds=27, read_backs=6, admitted=4, preempted=1, peak_pages=3)
    assert stats["admitted"] == len(out) + stats["preempted"]


def test_a_request_that_waits_while_nothing_runs_is_an_error():
    s = _sched([5], batch=1, pool=1)
    s.free = 0                                                           # (a state the loop cannot reach: every page taken, no row occupied)
    assert s.place() == ([], [])
    with pytest.raises(AssertionError, match="does not fit the empty pool"):
        s.idle()
