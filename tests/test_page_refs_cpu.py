"""The two numpy restatements of the reference-count rules (tests/_page_ref_cases.py) against each other and against the counted pool's
invariant, on the named cases, on hand-computed states and on a few hundred random op sequences - what tests/test_page_refs_gpu.py then
holds the kernels to."""
import numpy as np
import pytest

import _page_cases as P
import _page_ref_cases as R


def _run(B, mb, L, N, ops, broken=False):
    """Both forms through `ops`, compared after every op; the invariant behind every op that is no poke -> the states."""
    a = b = R.new_state(B, mb, L, N)
    cache, states, poked = set(), [], False
    for i, op in enumerate(ops):
        prev = a
        (a, fa), (b, fb) = R.apply_loop(a, op), R.apply_arrays(b, op)
        assert R.same_state(a, b) is None, (i, op["kind"], R.same_state(a, b))
        assert (fa is None and fb is None) or np.array_equal(fa, fb)
        poked = poked or op["kind"] == "poke"
        if broken and i == len(ops) - 1:
            assert a["error"] == 1 and R.same_state(dict(a, error=0), dict(prev, error=0)) is None
            assert fa is None or np.array_equal(fa, op["finished"])
        else:
            assert a["error"] == 0, (i, op["kind"])
            cache = R.cache_after(cache, op, False)
            if not poked:
                R.check_invariant(a, cache)
        states.append(a)
    return states


@pytest.mark.parametrize("name", sorted(R.named_cases()))
def test_named_cases_agree_and_keep_the_invariant(name):
    _run(*R.named_cases()[name], broken=name in R.BROKEN)


def test_broken_names_are_named_cases():
    assert set(R.BROKEN) <= set(R.named_cases())


def test_one_page_in_three_more_rows_by_hand():
    st = _run(*R.named_cases()["three_rows"])[-1]
    assert st["refs"].tolist() == [4, 2, 1, 1, 0, 0, 0] and st["owned"].tolist() == [2, 2, 1, 1, 2] and st["count"] == 3
    assert st["page_ids"][2:].tolist() == [[0, -1, -1, -1], [0, -1, -1, -1], [0, 1, -1, -1]]
    pb = st["page_bytes"]
    assert st["tables"][1, 4, 1].tolist() == [int(st["bases"][1, 1]) + p * pb for p in (0, 1, 7, 7)]


def test_a_shared_page_is_pushed_once_where_it_was_first_named():
    st = _run(*R.named_cases()["shared_released_together"])[-1]
    # H = row 1: 2, 3; row 2: 2; row 3: 3, 2 - both freed, 2 before 3, behind the three free pages 6, 5, 4
    assert st["count"] == 5 and st["free"][:5].tolist() == [6, 5, 4, 2, 3] and st["refs"].tolist() == [1, 1, 0, 0, 0, 0, 0]


def test_one_of_two_holders_pushes_nothing():
    states = _run(*R.named_cases()["one_of_two"])
    assert states[2]["count"] == 3 and states[2]["refs"][:2].tolist() == [1, 1]
    assert states[3]["count"] == 5 and states[3]["free"][3:5].tolist() == [0, 1]


def test_cache_and_row_in_either_order_and_together():
    states = _run(*R.named_cases()["cache_drops_first"])
    assert states[1]["refs"][:2].tolist() == [2, 2] and states[2]["count"] == 3 and states[3]["free"][3:5].tolist() == [0, 1]
    states = _run(*R.named_cases()["row_first"])
    assert states[2]["count"] == 3 and states[2]["owned"][0] == 0 and states[3]["free"][3:5].tolist() == [1, 0]
    states = _run(*R.named_cases()["row_and_cache_together"])
    # row 1 (pages 2, 3) let go: 2 is freed, 3 stays with the cache; then H = row 0: 0, 1; drops: 3, 1
    assert states[2]["free"][:4].tolist() == [6, 5, 4, 2] and states[3]["free"][4:7].tolist() == [0, 1, 3] and states[3]["count"] == 7


def test_a_reserve_grows_behind_a_hold():
    st = _run(*R.named_cases()["hold_then_grow"])[-1]
    assert st["page_ids"][3].tolist() == [0, 1, 4, -1] and st["owned"][3] == 3 and st["refs"].tolist() == [2, 2, 1, 1, 1, 0, 0]


def test_the_wide_cases_end_with_every_page_free():
    for name in ("wave", "stride", "chunk", "full", "many_freed"):
        st = _run(*R.named_cases()[name])[-1]
        assert st["count"] == st["N"] and not st["refs"].any(), name
    # many_freed: 233 rows of 3 pages; the rows' pages come back in row order, a cached one too (its drop comes later in H)
    assert st["free"][1:700].tolist() == list(range(699))


@pytest.mark.parametrize("seed", range(6))
def test_random_sequences_agree_and_keep_the_invariant(seed):
    rng = np.random.default_rng(seed)
    B, mb, N = [(5, 4, 7), (37, 5, 90), (9, 3, 12)][seed % 3]
    _run(B, mb, 2, N, R.random_ops(rng, B, mb, 2, N, 60))


def test_a_pool_that_never_shares_is_the_uncounted_pool():
    rng = np.random.default_rng(3)
    B, mb, N = 37, 5, 90
    ops = P.random_ops(rng, B, mb, 120)
    a, b = P.new_state(B, mb, 2, N), R.new_state(B, mb, 2, N)
    for op, cop in zip(ops, R.unshared_ops(np.random.default_rng(3), B, mb, 120)):
        (a, fa), (b, fb) = P.apply_loop(a, op), R.apply_loop(b, cop)
        assert P.same_state(a, b) is None and ((fa is None and fb is None) or np.array_equal(fa, fb))
        R.check_invariant(b)
        P.check_invariant(b)
