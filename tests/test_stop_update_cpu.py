"""The stop rule without a GPU: the two numpy restatements of tests/_stop_cases.py against each other on the GPU test's cases and on
random ones, hand-worked cases, `stopping.stop_table`, and the conditions the GPU case set has to meet so that the GPU test cannot pass
vacuously."""
import numpy as np
import pytest

from _stop_cases import NO_LIMIT, SENTINEL, _seq, assemble, gpu_cases, named_cases, random_case, restate_arrays, restate_loop, row, table


def _same(a, b, what):
    for key in a:
        assert np.array_equal(a[key], b[key]), f"{what}: {key}: {a[key].tolist()} != {b[key].tolist()}"


def test_the_two_restatements_agree():
    rng = np.random.default_rng(5)
    cases = list(gpu_cases().items()) + [(f"extra{i}", random_case(rng)) for i in range(300)]
    for name, case in cases:
        _same(restate_loop(case), restate_arrays(case), name)


def _one(r, stops, **kw):
    case = assemble([r], stops, **kw)
    out = restate_loop(case)
    _same(out, restate_arrays(case), r["name"])
    return tuple(int(out[k][0]) for k in ("accept_lens", "next_token", "last_row", "finished"))


def test_hand_worked_cases():
    T = table([[7], [3, 4]])
    text = [11, 12, 13, 14]
    kw = dict(n=6, cap=32)
    # the path 20, 7, 21 and the bonus 22: the 7 is e_2 - two tokens are emitted, the current token becomes the 7 of node 2, the last
    # accepted row is node 1
    assert _one(row("e2", text, [20, 7, 21], 22, plen=2), T, **kw) == (2, 7, 1, 1)
    # nothing stops: all four, and neither next_token nor last_row is written
    assert _one(row("none", text, [20, 21, 23], 22, plen=2), T, **kw) == (4, 22, SENTINEL, 0)
    # a limit of 6 tokens: L = 4, so e_2 is the last token (L + 2 >= 6); reason 2
    assert _one(row("limit", text, [20, 21, 23], 22, plen=2, limit=6), T, **kw) == (2, 21, 1, 2)
    # the limit and the stop fall on e_2: reason 1
    assert _one(row("both", text, [20, 7, 21], 22, plen=2, limit=6), T, **kw) == (2, 7, 1, 1)
    # [3, 4] over the seam: the 3 is the current token, the 4 is e_1; with the 3 still in the prompt the match does not count
    assert _one(row("seam", text + [3], [4, 20], 21, plen=4), T, **kw) == (1, 4, 0, 1)
    assert _one(row("prompt", text + [3], [4, 20], 21, plen=5), T, **kw) == (3, 21, SENTINEL, 0)
    # finished on entry: nothing is emitted, the token is the text's last, the reason stays
    assert _one(row("frozen", text, [7, 7], 7, fin=2), T, **kw) == (0, 14, SENTINEL, 2)
    # the current token is a stop: seen with check_root alone
    assert _one(row("root", text + [7], [20], 21), T, **kw) == (2, 21, SENTINEL, 0)
    assert _one(row("root", text + [7], [20], 21), T, check_root=1, **kw) == (0, 7, SENTINEL, 1)
    # a plain step: m = 1, the new token is e_1
    assert _one(row("step", text, bonus=7), T, n=1, cap=32, step=True) == (1, 7, SENTINEL, 1)
    assert _one(row("step", text, bonus=8, limit=4), T, n=1, cap=32, step=True) == (0, 14, SENTINEL, 2)


def test_the_gpu_case_set_is_not_vacuous():
    """With the restatement alone: over everything the GPU test launches, at least a quarter of the live rows are clipped inside their
    path (1 <= k < m), both finish reasons and the "stays live" outcome occur, and the 65th index of a 64-node path decides somewhere."""
    live = inside = 0
    reasons, index64 = set(), 0
    for case in gpu_cases().values():
        out = restate_loop(case)
        for b in range(len(case["lengths"])):
            if case["finished"][b] != 0:
                assert out["accept_lens"][b] == 0 and out["finished"][b] == case["finished"][b]
                continue
            _, m, _ = _seq(case, b)
            k = int(out["accept_lens"][b])
            live += 1
            inside += 1 <= k < m
            reasons.add(int(out["finished"][b]))
            index64 += k == 64 and out["finished"][b] != 0
    assert live >= 100 and 4 * inside >= live, f"{inside} of {live} live rows clip inside the path"
    assert reasons == {0, 1, 2}
    assert index64 >= 2


def test_every_named_case_is_there():
    names = [n for case in named_cases().values() for n in case["names"]]
    for part in ("seam", "begin inside the prompt", "stop at e_1", "stop at e_m", "none", "limit and stop on the same index", "limit before stop",
                 "L >= limit on entry", "already finished", "check_root hit", "turned-off rows", "S = 0", "S = 32, W = 8", "out of range",
                 "lengths beyond the cap"):
        assert any(part in n for n in names), part
    assert {case["n"] for case in named_cases().values()} >= {1, 12, 64}
    assert all(len(case["lengths"]) <= 8 for case in gpu_cases().values())


def test_stop_table(built_lib):
    from qserve_amd import stopping as S
    seqs, lens = S.stop_table([7, (3, 4), [9, 9, 9]])
    assert seqs.tolist() == [[7, -1, -1], [3, 4, -1], [9, 9, 9]] and lens.tolist() == [1, 2, 3]
    seqs, lens = S.stop_table([], num_rows=S.MAX_STOPS, width=S.MAX_STOP_LEN)
    assert tuple(seqs.shape) == (32, 8) and lens.tolist() == [0] * 32 and (S.MAX_STOPS, S.MAX_STOP_LEN) == (32, 8)
    assert S.stop_table([])[1].tolist() == [0]
    for bad in ([[]], [[1] * 9], [-1], [[1, -2]], list(range(33))):
        with pytest.raises(ValueError, match="stop_table"):
            S.stop_table(bad)
    with pytest.raises(ValueError, match="width"):
        S.stop_table([[1, 2, 3]], width=2)
    assert NO_LIMIT == 2 ** 31 - 1
