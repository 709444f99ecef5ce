"""The two numpy restatements of the fork rule (tests/_page_fork_cases.py) against each other, against the counted pool's invariant,
and against what the named cases say they show - what tests/test_page_fork_gpu.py then holds the kernels to."""
import numpy as np
import pytest

import _page_fork_cases as K


def _walk(B, mb, L, N, ops, broken=False, page_bytes=16):
    st = K.new_state(B, mb, L, N, page_bytes)
    cache, poked, states = set(), False, [st]
    for i, op in enumerate(ops):
        new, fin = K.apply_loop(st, op)
        other, other_fin = K.apply_arrays(st, op)
        assert K.same_state(new, other) is None, (i, op["kind"], K.same_state(new, other))
        assert (fin is None and other_fin is None) or np.array_equal(fin, other_fin), (i, op["kind"])
        poked = poked or op["kind"] == "poke"
        if broken and i == len(ops) - 1:
            assert new["error"] == 1
            new["error"] = st["error"]
            assert K.same_state(new, st) is None                            # nothing else changed, no byte either
            assert fin is None or np.array_equal(fin, op["finished"])
        else:
            assert new["error"] == 0, (i, op["kind"])
            cache = K.cache_after(cache, op, False)
            if not poked:
                K.check_invariant(new, cache)
        st = new
        states.append(st)
    return states


@pytest.mark.parametrize("name", sorted(K.named_cases()))
def test_loop_and_arrays_agree_on_every_named_case(name):
    _walk(*K.named_cases()[name], broken=name in K.BROKEN)


@pytest.mark.parametrize("seed,shape", [(0, (5, 4, 7)), (1, (37, 5, 90)), (2, (9, 3, 12)), (3, (70, 6, 300))])
def test_loop_and_arrays_agree_on_random_sequences(seed, shape):
    B, mb, N = shape
    ops = K.random_ops(np.random.default_rng(seed), B, mb, 3, N, 80)
    states = _walk(B, mb, 3, N, ops)
    forks = [(a, b, op) for a, b, op in zip(states, states[1:], ops) if op["kind"] == "fork"]
    assert len(forks) >= 8
    # the stream is worth running: forks that share, forks that copy, forks that are refused
    assert any((b["refs"] > 1).sum() > (a["refs"] > 1).sum() for a, b, _ in forks)
    assert any(not np.array_equal(a["bytes"], b["bytes"]) for a, b, _ in forks)
    assert any(b["starved"].sum() > a["starved"].sum() for a, b, _ in forks)


def _last(name):
    B, mb, L, N, ops = K.named_cases()[name]
    states = _walk(B, mb, L, N, ops)
    return states, ops


def test_what_the_boundary_cases_show():
    for name, owned, free, copied in (("t0", [3, 2, 2, 0, 0], 4, 0), ("t1", [3, 3, 0, 0, 0], 3, 1), ("t63", [2, 0, 0, 2, 0], 4, 1),
                                      ("len1", [1, 1, 0, 0, 0], 5, 0)):
        states, _ = _last(name)
        before, st = states[-2], states[-1]
        assert st["owned"].tolist() == owned and st["count"] == free, name
        pages = np.nonzero((before["bytes"] != st["bytes"]).any(axis=(0, 1, 3)))[0]
        assert len(pages) == copied, name
    st = _last("t1")[0][-1]
    assert st["page_ids"][1].tolist() == [0, 1, 3, -1] and st["refs"][:4].tolist() == [2, 2, 1, 1]
    assert np.array_equal(st["bytes"][:, :, 3], st["bytes"][:, :, 2])
    st = _last("one_into_many")[0][-1]
    assert st["refs"].tolist() == [5, 1, 1, 1, 1, 1, 0] and st["page_ids"][:, 1].tolist() == [1, 2, 3, 4, 5] and st["count"] == 1
    for j in (2, 3, 4, 5):
        assert np.array_equal(st["bytes"][:, :, j], st["bytes"][:, :, 1])
    st = _last("two_sources")[0][-1]
    assert st["page_ids"].tolist() == [[0, 1, -1, -1], [0, 5, -1, -1], [2, 3, 6, -1], [2, 3, 4, -1], [2, 3, 7, -1]]


def test_rows_are_served_in_order_while_the_free_pages_last():
    states, ops = _last("free_ends_midway")
    st = states[-1]
    assert st["owned"].tolist() == [2, 3, 2, 2, 0, 0, 2] and st["starved"].tolist() == [0, 0, 0, 0, 1, 1, 0] and st["count"] == 0
    assert st["page_ids"][6].tolist() == [2, 3, -1, -1]                     # t = 0 behind two refused rows: served, nothing popped
    new, fin = K.apply_loop(states[1], K.named_cases()["free_ends_midway_finished"][4][1])
    assert fin.tolist() == [0, 0, 0, 2, K.NO_PAGES, 1, 0] and K.same_state(new, st) is None


def test_a_starved_source_refuses_its_destinations_without_an_error():
    states, ops = _last("starved_source")
    st = states[2]
    assert st["error"] == 0 and st["starved"].tolist() == [0, 0, 1, 0, 0] and st["owned"].tolist() == [1, 1, 0, 1, 1]
    assert K.apply_loop(states[1], ops[1])[1].tolist() == [0, 0, K.NO_PAGES, 0, 0]
    assert K.same_state(states[3], st) is None                              # beyond max_blocks: refused again, nothing moves


def test_the_wide_cases_cross_a_wave_and_the_stride_and_run_out_of_pages():
    for name, B in (("wave", 70), ("stride", 300), ("chunk", 256), ("full", 1024)):
        states, ops = _last(name)
        st = states[2]
        dests = np.nonzero(ops[1]["src_rows"] >= 0)[0]
        assert len(dests) == B - (B + 2) // 3
        refused = st["starved"][dests] != 0
        assert refused.any() and not refused.all() and st["count"] == 0
        assert (st["owned"][dests[~refused]] > 0).any() and states[-1]["count"] == st["N"]
