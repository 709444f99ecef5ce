"""The rules of `qs_beam_select`'s second launch and of `qs_rows_move` (include/qserve_amd.h) on their restatements alone, without a GPU:
the named cases of tests/_beam_cases.py hold the situations the contract names, every result is a bijection of the chosen candidates
onto slots whose moves have sources that stay, and (moved, src_rows) pass through the restated page pool - unhold, then fork - without
breaking an invariant."""
import numpy as np
import pytest

import _beam_cases as K
import _page_fork_cases as F

CASES = K.named_cases()


def _merged(case):
    """The restatement over the float64 oracle's candidate lists, rounded to fp32 (what launch 1 would hand over, up to its error)."""
    ids, lp = K.candidates_oracle(case["logits"], case["cum"], case["finished"], case["W"])
    return ids, lp.astype(np.float32), K.merge_loop(case["cum"], case["finished"], case["tokens"], ids, lp.astype(np.float32), case["W"])


def _check_result(inp, res):
    """Bijection onto slots, sources that stay, the slot rule, and the page pool's preconditions."""
    W, cum, fin, tokens, ids, lp = inp["W"], inp["cum"], inp["finished"], inp["tokens"], inp["cand_ids"], inp["cand_lp"]
    B = cum.size
    parent, nxt, out = res["parent"], res["next_token"], res["cum_out"]
    assert np.array_equal(parent[parent], parent), "a source of a move is itself a destination"
    assert np.array_equal(res["moved"], (parent != np.arange(B)).astype(np.int32))
    assert np.array_equal(res["src_rows"], np.where(parent != np.arange(B), parent, -1))
    for g in range(B // W):
        rows = range(g * W, g * W + W)
        cands = K.group_candidates(g, cum, fin, tokens, ids, lp, W, lambda a, b: np.float32(a) + np.float32(b))
        chosen = cands[:W]
        filled = [d for d in rows if out[d] != K.NEG]
        # every chosen candidate sits in exactly one slot of its group, and nothing else does
        got = sorted((int(parent[d]), int(nxt[d]), np.float32(out[d]).tobytes()) for d in filled)
        assert got == sorted((b, t, np.float32(s).tobytes()) for s, b, _, t in chosen) and len(filled) == len(chosen)
        assert all(g * W <= parent[d] < g * W + W for d in rows)
        first = {}
        for c in chosen:
            first.setdefault(c[1], c)
        for p, c in first.items():                                          # a row with a chosen candidate keeps its best one
            assert parent[p] == p and nxt[p] == c[3] and np.float32(out[p]).tobytes() == np.float32(c[0]).tobytes()
        for d in rows:
            if d not in filled:                                             # a slot left over
                assert parent[d] == d and nxt[d] == tokens[d]
        rest = [c for c in chosen if first[c[1]] is not c]
        holes = [d for d in rows if d not in first]
        for c, d in zip(rest, holes):                                       # further children, in order, into the holes, ascending
            assert parent[d] == c[1] and nxt[d] == c[3]


def _through_the_pool(res, lengths, finished):
    """A pool in which every row holds the pages of its text: unhold(moved), then fork(src_rows), as the beam round issues them."""
    B = res["parent"].size
    mb = 4
    pages = int(sum(-(-int(n) // 64) for n in lengths))
    st = F.new_state(B, mb, 1, pages + B, page_bytes=8)
    st, _ = F.apply_loop(st, F._texts(B, {b: int(n) for b, n in enumerate(lengths)}))
    assert st["error"] == 0 and not st["starved"].any()
    F.check_invariant(st)
    st, _ = F.apply_loop(st, F._unhold(res["moved"]))
    assert st["error"] == 0
    F.check_invariant(st)
    st, fin = F.apply_loop(st, dict(kind="fork", src_rows=res["src_rows"], lengths=np.asarray(lengths, np.int32),
                                    finished=np.asarray(finished, np.int32)))
    assert st["error"] == 0, "the fork met a broken invariant: a destination that owns pages, or a source that is a destination"
    F.check_invariant(st)
    assert not st["starved"].any()                                          # (the pool has a page per row to spare)
    for d in np.nonzero(res["moved"])[0]:
        p = res["parent"][d]
        w = (max(int(lengths[p]), 1) - 1) // 64
        assert np.array_equal(st["page_ids"][d, :w], st["page_ids"][p, :w])
    assert np.array_equal(fin, finished)


def _inp(case, ids, lp):
    return dict(W=case["W"], cum=case["cum"], finished=case["finished"], tokens=case["tokens"], cand_ids=ids, cand_lp=lp)


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_case_is_a_bijection_whose_moves_the_pool_accepts(name):
    case = CASES[name]
    ids, lp, res = _merged(case)
    _check_result(_inp(case, ids, lp), res)
    B = case["cum"].size
    lengths = [(61 * b) % 200 + 2 for b in range(B)]                         # t = 0, t > 0 and several pages all occur
    _through_the_pool(res, lengths, case["finished"])


def test_1000_random_inputs():
    rng = np.random.default_rng(2024)
    moved = taken_all = identity = 0
    for _ in range(1000):
        inp = K.random_merge_input(rng)
        res = K.merge_loop(inp["cum"], inp["finished"], inp["tokens"], inp["cand_ids"], inp["cand_lp"], inp["W"])
        _check_result(inp, res)
        B = inp["cum"].size
        _through_the_pool(res, rng.integers(1, 250, size=B), inp["finished"])
        moved += int(res["moved"].any())
        identity += int(not res["moved"].any())
        taken_all += int(inp["W"] > 1 and any(len(set(res["parent"][g * inp["W"]:(g + 1) * inp["W"]])) == 1 and
                                               (res["cum_out"][g * inp["W"]:(g + 1) * inp["W"]] != K.NEG).all()
                                               for g in range(B // inp["W"])))
    assert moved > 100 and identity > 100 and taken_all > 5, (moved, identity, taken_all)


# ---- the situations the contract names, each on the restatement alone -----------------------------------------------------------------
def test_all_equal_logits_are_cut_by_index():
    ids, lp, res = _merged(CASES["all_equal"])
    assert np.array_equal(ids, np.tile(np.arange(4), (4, 1)))               # every row lists its first W ids
    assert np.array_equal(res["parent"], [0, 0, 0, 0]) and np.array_equal(res["next_token"], [0, 1, 2, 3])
    ids, lp, res = _merged(CASES["all_equal_g3_n9"])
    assert np.array_equal(res["parent"], [0, 0, 0, 3, 3, 3, 6, 6, 6]) and np.array_equal(res["next_token"], [0, 1, 2] * 3)


def test_fewer_than_w_listable_logits_leave_tails_that_are_no_candidates():
    case = CASES["few_listable"]
    ids, lp, res = _merged(case)
    assert (ids[:, 3:] == -1).all() and (ids[:, :3] >= 0).all() and np.isneginf(lp[:, 3:]).all()
    assert set(res["next_token"].tolist()) <= {1, 4, 8} and (res["cum_out"] != K.NEG).all()


def test_dead_rows_are_no_parents_and_give_their_slots_away():
    case = CASES["dead_rows"]
    ids, lp, res = _merged(case)
    dead = np.nonzero(case["cum"] == K.NEG)[0]
    assert (ids[dead] == -1).all()
    assert not np.isin(res["parent"], dead).any() and (res["cum_out"] != K.NEG).all()
    assert res["moved"][dead].all()


def test_frozen_rows_compete_with_their_sum_and_keep_their_token():
    case = CASES["frozen_rows"]
    ids, lp, res = _merged(case)
    frozen = np.nonzero(case["finished"])[0]
    assert (ids[frozen] == -1).all()
    for d in range(6):
        p = res["parent"][d]
        if case["finished"][p]:
            assert d == p and res["next_token"][d] == case["tokens"][p] and res["cum_out"][d] == case["cum"][p]
    assert res["parent"][1] == 1 or not np.isin(1, res["parent"])          # a frozen row has one candidate: it stays or it is dropped
    case = CASES["all_frozen_group"]
    ids, lp, res = _merged(case)
    assert np.array_equal(res["parent"][:3], [0, 1, 2]) and np.array_equal(res["cum_out"][:3], case["cum"][:3])
    assert np.array_equal(res["next_token"][:3], case["tokens"][:3]) and not res["moved"][:3].any()


def test_a_frozen_row_that_wins_stays_in_its_slot():
    case = CASES["frozen_wins"]
    ids, lp, res = _merged(case)
    assert res["parent"][1] == 1 and res["cum_out"][1] == np.float32(-0.25) and res["next_token"][1] == case["tokens"][1]
    assert res["cum_out"].max() == np.float32(-0.25) and np.count_nonzero(res["parent"] == 1) == 1


def test_equal_scores_across_rows_go_by_row_then_place():
    ids, lp, res = _merged(CASES["equal_across_rows"])
    # three identical rows: the best token of rows 0, 1, 2 ties three ways and fills the group, every row keeps its own
    assert np.array_equal(res["parent"], [0, 1, 2]) and len(set(res["next_token"].tolist())) == 1
    assert len({np.float32(s).tobytes() for s in res["cum_out"]}) == 1
    case = CASES["equal_with_frozen"]
    ids, lp, res = _merged(case)
    # row 0 live: 8 equal continuations at -2 log 8; row 1 frozen at -log 8 wins; then (0, 0): both keep their slots
    assert np.array_equal(res["parent"], [0, 1]) and res["next_token"][0] == 0 and res["next_token"][1] == case["tokens"][1]
    ids, lp, res = _merged(CASES["signed_zero"])
    assert np.array_equal(res["parent"], [0, 1]) and np.signbit(res["cum_out"][0]) and res["cum_out"][1] == 0


@pytest.mark.parametrize("name,row", [("one_parent_takes_all", 3), ("one_parent_takes_all_w32", 31)])
def test_one_parent_takes_all_w(name, row):
    case = CASES[name]
    ids, lp, res = _merged(case)
    W = case["W"]
    assert (res["parent"] == row).all() and res["moved"].sum() == W - 1
    # its best child stays, the others fill rows 0, 1, .. in the order of the list
    assert res["next_token"][row] == ids[row, 0]
    assert np.array_equal(res["next_token"][np.arange(W) != row], ids[row, 1:])


@pytest.mark.parametrize("name", ["identity", "identity_w32"])
def test_every_parent_taking_exactly_one_is_the_identity(name):
    case = CASES[name]
    ids, lp, res = _merged(case)
    B = case["cum"].size
    assert np.array_equal(res["parent"], np.arange(B)) and not res["moved"].any() and (res["src_rows"] == -1).all()
    assert np.array_equal(res["next_token"], ids[:, 0])


def test_a_group_with_fewer_than_w_candidates_leaves_slots_over():
    case = CASES["fewer_than_w"]
    ids, lp, res = _merged(case)
    # candidates: the frozen row 1 and row 3's two listable tokens; rows 0 and 2 are dead: slot 0 takes row 3's second, slot 2 is left
    assert np.array_equal(res["parent"], [3, 1, 2, 3]) and np.array_equal(res["next_token"], [5, case["tokens"][1], case["tokens"][2], 2])
    assert res["cum_out"][2] == K.NEG and np.array_equal(res["moved"], [1, 0, 0, 0]) and np.array_equal(res["src_rows"], [3, -1, -1, -1])
    res = _merged(CASES["no_candidates"])[2]
    assert np.array_equal(res["parent"], [0, 1]) and (res["cum_out"] == K.NEG).all()
    assert np.array_equal(res["next_token"], CASES["no_candidates"]["tokens"])


def test_the_case_list_covers_the_shapes():
    seen = {(c["W"], c["cum"].size // c["W"], c["logits"].shape[1]) for c in CASES.values()}
    assert {w for w, _, _ in seen} == {1, 2, 3, 4, 7, 32} and {g for _, g, _ in seen} >= {1, 3}
    assert {n for _, _, n in seen} == {8, 9, 1000, 128256}


@pytest.mark.parametrize("name", K.gap_cases(CASES))
def test_gap_cases_have_the_gap_on_the_oracle_alone(name):
    """The W-th and the (W + 1)-th exact score differ by more than twice the bound of a score: qs_logprob_rows' own lp bound 1e-5 +
    2^-21 |lp|, and the one fp32 rounding of the sum on top."""
    assert K.gap_holds(CASES[name])
    case = CASES[name]
    cum = case["cum"].astype(np.float64)
    for cands in K.exact_scores(case):
        if len(cands) > case["W"]:
            lp_bound = max(1e-5 + 2.0 ** -21 * abs(s - cum[b]) for s, b, _, _ in cands)
            assert cands[case["W"] - 1][0] - cands[case["W"]][0] > 2 * lp_bound


# ---- the row move ---------------------------------------------------------------------------------------------------------------------
def test_move_loop_moves_rows_and_refuses_chains():
    t = [np.arange(12, dtype=np.int32).reshape(3, 4), np.array([10, 20, 30], np.int64)]
    out, err = K.move_loop([0, 0, 2], t)
    assert err == 0 and np.array_equal(out[0][1], t[0][0]) and np.array_equal(out[1], [10, 10, 30])
    out, err = K.move_loop([1, 2, 2], t)                                    # row 0 <- row 1, which is itself a destination
    assert err == 1 and np.array_equal(out[0][0], t[0][0]) and np.array_equal(out[0][1], t[0][2]) and np.array_equal(out[1], [10, 30, 30])
    out, err = K.move_loop([3, 1, -1], t)
    assert err == 1 and all(np.array_equal(a, b) for a, b in zip(out, t))
