"""The two numpy restatements of the page pool rules (tests/_page_cases.py) against each other and against the pool's invariant, on the
named cases, on hand-computed states and on random op sequences - what tests/test_page_pool_gpu.py then holds the kernels to."""
import numpy as np
import pytest

import _page_cases as P
from qserve_amd.stopping import NO_PAGES                                    # the reason the restatements give a refused row: the engine's

assert NO_PAGES == P.NO_PAGES


def _run(B, mb, L, N, ops, check=True):
    """Both forms through `ops`, compared after every op -> the states and the `finished` arrays behind each op."""
    a = b = P.new_state(B, mb, L, N)
    states, fins = [], []
    for op in ops:
        (a, fa), (b, fb) = P.apply_loop(a, op), P.apply_arrays(b, op)
        assert P.same_state(a, b) is None, (op["kind"], P.same_state(a, b))
        assert (fa is None and fb is None) or np.array_equal(fa, fb)
        if check:
            P.check_invariant(a)
        states.append(a)
        fins.append(fa)
    return states, fins


@pytest.mark.parametrize("name", sorted(P.named_cases()))
def test_named_cases_agree_and_keep_the_invariant(name):
    _run(*P.named_cases()[name])


def test_the_boundary_lengths_by_hand():
    """lengths 64, 65, 1, 128, 129 over 7 pages: a step needs 1, 2, 1, 2, 3 pages, a 12-node tree 2, 2, 1, 3, 3."""
    (st,), _ = _run(*P.named_cases()["step"])
    assert st["owned"].tolist() == [1, 2, 1, 2, 0] and st["starved"].tolist() == [0, 0, 0, 0, 1] and st["count"] == 1
    assert st["page_ids"][:4].tolist() == [[0, -1, -1, -1], [1, 2, -1, -1], [3, -1, -1, -1], [4, 5, -1, -1]]
    assert st["free"][:1].tolist() == [6]
    (st,), _ = _run(*P.named_cases()["tree12"])
    assert st["owned"].tolist() == [2, 2, 1, 0, 0] and st["starved"].tolist() == [0, 0, 0, 1, 1] and st["count"] == 2
    pb, N = st["page_bytes"], st["N"]
    assert st["tables"][1, 1, 1].tolist() == [int(st["bases"][1, 1]) + p * pb for p in (2, 3, N, N)]


def test_a_middle_row_starves_and_the_rest_goes_on():
    states, _ = _run(*P.named_cases()["middle_starves"])
    st = states[-1]
    assert st["owned"].tolist() == [1, 1, 1, 1, 1] and st["starved"].tolist() == [0, 1, 0, 0, 1] and st["count"] == 2


def test_finished_rows_do_not_grow_and_starved_rows_take_the_reason():
    (st,), (fin,) = _run(*P.named_cases()["finished_mask"])
    assert st["owned"].tolist() == [4, 0, 2, 0, 0] and st["starved"].tolist() == [0, 0, 0, 1, 1]
    assert fin.tolist() == [0, 2, 0, P.NO_PAGES, P.NO_PAGES] and st["count"] == 1


def test_released_pages_come_back_last_pushed_first():
    states, _ = _run(*P.named_cases()["release_reuse"])
    assert states[1]["free"][:4].tolist() == [1, 2, 4, 5] and states[1]["count"] == 4
    st = states[2]
    assert st["page_ids"][1, 0] == 5 and st["page_ids"][2, :3].tolist() == [3, 4, 2] and st["page_ids"][3, 0] == 1
    assert st["starved"].tolist() == [0, 0, 0, 0, 1] and st["count"] == 0
    assert states[3]["count"] == 7 and (states[3]["page_ids"] == -1).all()


def test_extra_rows_is_the_prompt_of_an_admission():
    states, _ = _run(*P.named_cases()["extra_rows"])
    assert states[0]["owned"].tolist() == [2, 0, 0, 0, 0]
    assert states[1]["owned"].tolist() == [2, 3, 0, 1, 0] and states[1]["starved"].tolist() == [0, 0, 0, 0, 1]


@pytest.mark.parametrize("seed", range(6))
def test_random_op_sequences(seed):
    rng = np.random.default_rng(seed)
    B, mb = int(rng.integers(1, 40)), int(rng.integers(1, 6))
    N = int(rng.integers(1, B * mb + 2))
    _run(B, mb, 2, N, P.random_ops(rng, B, mb, 60))


def test_broken_invariants_set_error_and_change_nothing():
    base = _run(5, 4, 2, 7, [P.named_cases()["step"][4][0]])[0][0]
    op, rel = P.named_cases()["tree12"][4][0], dict(kind="release", mask=np.ones((5,), np.int32))
    for key, at, value in (("count", None, 8), ("count", None, -1), ("owned", 2, 5), ("owned", 0, -1)):
        bad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()}
        if at is None:
            bad[key] = value
        else:
            bad[key][at] = value
        for apply in (P.apply_loop, P.apply_arrays):
            for o in (op, rel):
                out, _ = apply(bad, o)
                assert out["error"] == 1
                for k in ("free", "count", "page_ids", "owned", "starved", "tables"):
                    assert np.array_equal(out[k], bad[k]), (key, k)
    bad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()}
    bad["free"][0] = 7                                                       # the page a growing row 0 would pop
    grow0 = dict(kind="reserve", lengths=np.asarray([65, 1, 1, 1, 1], np.int32), extra=1, extra_rows=None, finished=None)
    for apply in (P.apply_loop, P.apply_arrays):
        assert apply(bad, grow0)[0]["error"] == 1
    bad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()}
    bad["page_ids"][1, 1] = -3
    for apply in (P.apply_loop, P.apply_arrays):
        assert apply(bad, rel)[0]["error"] == 1
