"""Beam selection (`qs_beam_select`, `qs_rows_move`; include/qserve_amd.h) restated: launch 2 and the row move as loops over exactly the
operations the header names - one fp32 addition per score, an integer order -, launch 1 as a float64 oracle (tests/_logprob_cases.py:
log-softmax, the top W by fp16 key, then index), and the named cases of tests/test_beam_select_*.py.

A CASE is a dict: logits fp16 [B, n], cum float32 [B], finished int32 [B], tokens int64 [B], W, and `gap`: whether the W-th and the
(W + 1)-th exact score of every group lie further apart than the kernels' arithmetic can move them, so that the chosen set is
decided by the float64 oracle alone."""
import functools

import numpy as np

import _logprob_cases as L

NEG = np.float32(-np.inf)


# ---- launch 1: the float64 oracle ---------------------------------------------------------------------------------------------------------
def candidates_oracle(logits, cum, finished, W):
    """-> (ids int64 [B, W], lp float64 [B, W]) by the contract: a live row's top list, -1 / -inf for a dead or frozen row."""
    B = logits.shape[0]
    ids, lp = np.full((B, W), -1, np.int64), np.full((B, W), -np.inf)
    for b in range(B):
        if cum[b] == NEG or finished[b] != 0:
            continue
        _, _, i, l = L.score(logits[b], -1, 1.0, W)
        ids[b], lp[b] = i, l
    return ids, lp


# ---- launch 2: the loop restatement -------------------------------------------------------------------------------------------------------
def group_candidates(g, cum, finished, tokens, cand_ids, cand_lp, W, add):
    """The candidates of group g as (score, row, r, token), dropped ones left out, in the order of the contract.  `add`: the addition."""
    cands = []
    for b in range(g * W, g * W + W):
        c = cum[b]
        if c == NEG:
            continue
        if finished[b] != 0:
            cands.append((c, b, 0, int(tokens[b])))
            continue
        for r in range(W):
            if cand_ids[b, r] >= 0:
                cands.append((add(c, cand_lp[b, r]), b, r, int(cand_ids[b, r])))
    cands = [c for c in cands if c[0] > -np.inf]                            # (-inf and NaN are dropped)
    return sorted(cands, key=lambda c: (-float(c[0]), c[1], c[2]))          # (-0.0 == +0.0 as floats)


def merge_loop(cum, finished, tokens, cand_ids, cand_lp, W):
    """-> dict(parent int32, next_token int64, cum_out float32, moved int32, src_rows int32), slot by slot as the header words it."""
    cum, cand_lp = np.asarray(cum, np.float32), np.asarray(cand_lp, np.float32)
    B = cum.size
    assert B % W == 0
    parent, nxt, out = np.arange(B, dtype=np.int32), np.asarray(tokens, np.int64).copy(), np.full((B,), NEG, np.float32)
    for g in range(B // W):
        chosen = group_candidates(g, cum, finished, tokens, cand_ids, cand_lp, W, lambda a, b: np.float32(a) + np.float32(b))[:W]
        slot, rest = {}, []
        for c in chosen:
            if c[1] in slot:
                rest.append(c)
            else:
                slot[c[1]] = c
        holes = [d for d in range(g * W, g * W + W) if d not in slot]
        assert len(rest) <= len(holes)
        slot.update(zip(holes, rest))
        for d, (score, b, _, token) in slot.items():
            parent[d], nxt[d], out[d] = b, token, score
    moved = (parent != np.arange(B)).astype(np.int32)
    return dict(parent=parent, next_token=nxt, cum_out=out, moved=moved, src_rows=np.where(moved != 0, parent, -1).astype(np.int32))


def exact_scores(case):
    """Per group the float64 candidates (score, row, r, token) in order, from the oracle's lists."""
    ids, lp = candidates_oracle(case["logits"], case["cum"], case["finished"], case["W"])
    cum = case["cum"].astype(np.float64)
    return [group_candidates(g, cum, case["finished"], case["tokens"], ids, lp, case["W"], lambda a, b: a + b)
            for g in range(cum.size // case["W"])]


def score_bound(score, lp):
    """What the device's fp32 score may differ from the exact one by: the lp bound of qs_logprob_rows and the one rounding of the sum."""
    return L.TOL(lp) + 2.0 ** -24 * abs(score)


def gap_holds(case):
    """Is the W-th exact score of every group further from the (W + 1)-th than twice the largest bound of a candidate's score?"""
    W, cum = case["W"], case["cum"].astype(np.float64)
    for cands in exact_scores(case):
        if len(cands) <= W:
            continue
        slack = max(score_bound(s, s - cum[b]) for s, b, _, _ in cands)
        if not cands[W - 1][0] - cands[W][0] > 2 * slack:
            return False
    return True


# ---- the row move ---------------------------------------------------------------------------------------------------------------------
def move_loop(parent, tensors):
    """-> (the tensors after the move, error): row d becomes row parent[d]; a parent outside the batch or itself a destination is an
    error and skips the row."""
    parent = np.asarray(parent, np.int64)
    B, error = parent.size, 0
    out = [np.array(t, copy=True) for t in tensors]
    for d in range(B):
        p = int(parent[d])
        if p == d:
            continue
        if not 0 <= p < B or parent[p] != p:
            error = 1
            continue
        for o, t in zip(out, tensors):
            o[d] = t[p]
    return out, error


# ---- the named cases ----------------------------------------------------------------------------------------------------------------------
def _case(logits, cum, W, finished=None, tokens=None, gap=False):
    logits = np.ascontiguousarray(logits, np.float16)
    B = logits.shape[0]
    assert B % W == 0 and len(cum) == B
    return dict(logits=logits, cum=np.asarray(cum, np.float32), W=W, gap=gap,
                finished=np.zeros((B,), np.int32) if finished is None else np.asarray(finished, np.int32),
                tokens=(np.arange(B, dtype=np.int64) * 3 + 1) % logits.shape[1] if tokens is None else np.asarray(tokens, np.int64))


def _random(seed, W, G, n, spread=3.0):
    rng = np.random.default_rng(seed)
    B = W * G
    return _case(rng.normal(size=(B, n)) * spread, -rng.random(B) * 4, W, gap=True)


def _gapped(W, G, n):
    """The first seed whose random case has the gap (random fp16 rows hold ties: not every seed has it)."""
    for seed in range(200):
        case = _random(1000 * W + 10 * G + seed * 7919 + n, W, G, n)
        if gap_holds(case):
            return case
    raise AssertionError(f"no gapped case for W={W}, G={G}, n={n}")


def _peaked(B, n, at, high=12.0, low=-12.0):
    x = np.full((B, n), low)
    for b in range(B):
        x[b, at(b)] = high
    return x


@functools.lru_cache(maxsize=None)
def named_cases():
    """name -> case; computed once and shared: nobody writes into a case."""
    inf = np.inf
    cases = {}
    for W in (1, 2, 3, 4, 7, 32):
        for G, n in ((1, 8), (3, 9), (1, 1000), (3, 1000)):
            if W == 32 and G == 3 and n == 1000:
                continue                                                    # (the oracle's time; W = 32 meets G = 3 at n = 9)
            cases[f"random_w{W}_g{G}_n{n}"] = _gapped(W, G, n)
    # all logits equal, all scores equal: every tie is cut by index - row 0's first W ids win, rows 1 .. W - 1 become its children
    cases["all_equal"] = _case(np.full((4, 8), 0.5), [-1.0] * 4, 4)
    cases["all_equal_g3_n9"] = _case(np.full((9, 9), -2.0), [-0.5] * 9, 3)
    # 3 listable logits per row for W = 7: tails of id -1 that are no candidates
    x = np.full((7, 9), -inf)
    x[:, [1, 4, 8]] = np.random.default_rng(3).normal(size=(7, 3))
    cases["few_listable"] = _case(x, -np.arange(7) * 0.25, 7)
    # dead rows: never a parent, their slots go to further children of the live rows
    cases["dead_rows"] = _case(np.random.default_rng(4).normal(size=(8, 1000)) * 2, [-1.0, -inf, -inf, -2.0, -inf, -inf, -inf, -0.5], 4)
    # frozen rows compete with their sum alone and keep their token
    cases["frozen_rows"] = _case(np.random.default_rng(5).normal(size=(6, 9)) * 2, [-1.0, -2.5, -0.5, -3.0, -1.0, -9.0], 3,
                                 finished=[0, 1, 0, 2, 0, 3])
    cases["all_frozen_group"] = _case(np.random.default_rng(6).normal(size=(6, 8)), [-1.0, -2.0, -3.0, -1.0, -2.0, -0.5], 3,
                                      finished=[1, 2, 1, 0, 0, 0])
    # a frozen row far ahead of every live continuation: it is chosen first and stays in its slot
    cases["frozen_wins"] = _case(np.random.default_rng(7).normal(size=(4, 1000)) * 3, [-30.0, -0.25, -30.0, -31.0], 4, finished=[0, 1, 0, 0])
    # identical rows with identical sums: equal scores across rows, row ascending decides
    cases["equal_across_rows"] = _case(np.tile(np.random.default_rng(8).normal(size=(1, 9)) * 2, (3, 1)), [-1.5] * 3, 3)
    cases["equal_with_frozen"] = _case(np.zeros((2, 8)), [-np.log(8.0), -np.log(8.0)], 2, finished=[0, 1])
    # one parent far ahead takes all W slots
    cases["one_parent_takes_all"] = _case(np.random.default_rng(9).normal(size=(7, 1000)), [-40.0] * 3 + [-1.0] + [-40.0] * 3, 7, gap=True)
    cases["one_parent_takes_all_w32"] = _case(np.random.default_rng(10).normal(size=(32, 1000)), [-60.0] * 31 + [-1.0], 32)
    # every row's best continuation is far ahead of every second one: the identity, nothing moves
    cases["identity"] = _case(_peaked(12, 9, lambda b: (b * 5) % 9), -np.arange(12) * 0.125, 4, gap=True)
    cases["identity_w32"] = _case(_peaked(32, 1000, lambda b: (b * 37) % 1000), -np.arange(32) * 0.0625, 32, gap=True)
    # fewer than W candidates in the group: two dead rows, a frozen one and a live one with two listable logits - one slot is left over
    x = np.full((4, 8), -inf)
    x[:, [2, 5]] = [1.0, 0.5]
    cases["fewer_than_w"] = _case(x, [-inf, -1.0, -inf, -2.0], 4, finished=[0, 1, 0, 0])
    cases["no_candidates"] = _case(np.zeros((2, 8)), [-inf, -inf], 2, finished=[0, 1])
    # -0.0 and +0.0 are one score: the frozen row 0 (sum -0.0) is equal to row 1's (+0.0), row ascending decides
    cases["signed_zero"] = _case(_peaked(2, 8, lambda b: 3, high=60.0, low=-60.0), [-0.0, 0.0], 2, finished=[1, 0])
    # one live row of Llama-3's vocabulary among dead ones
    big = np.random.default_rng(11).normal(size=(4, 128256)) * 3
    cases["big_row"] = _case(big, [-1.0, -inf, -inf, -inf], 4, gap=True)
    return cases


def gap_cases(cases):
    return [name for name, c in cases.items() if c["gap"]]


def random_merge_input(rng):
    """One seeded input of launch 2 alone: candidate lists as launch 1 could have left them (per live row lp descending, a tail of -1),
    coarse values so that ties across rows are common, dead and frozen rows mixed in."""
    W = int(rng.choice([1, 2, 3, 4, 7, 32]))
    G = int(rng.integers(1, 4))
    B = W * G
    state = rng.choice(3, size=B, p=[0.6, 0.2, 0.2])                        # live, frozen, dead
    cum = np.where(state == 2, -np.inf, -rng.integers(0, 8, size=B) * 0.5).astype(np.float32)
    cum = np.where((state != 2) & (rng.random(B) < 0.05), np.float32(-0.0), cum).astype(np.float32)
    finished = np.where(state == 1, rng.integers(1, 4, size=B), 0).astype(np.int32)
    finished = np.where((state == 2) & (rng.random(B) < 0.5), 1, finished).astype(np.int32)
    ids, lp = np.full((B, W), -1, np.int32), np.full((B, W), -np.inf, np.float32)
    for b in range(B):
        if state[b] != 0:
            continue
        k = int(rng.integers(0, W + 1)) if rng.random() < 0.3 else W
        ids[b, :k] = rng.permutation(50)[:k] if k <= 50 else np.arange(k)
        lp[b, :k] = -np.sort(rng.integers(0, 12, size=k)) * 0.25
    return dict(W=W, cum=cum, finished=finished, tokens=rng.integers(0, 50, size=B).astype(np.int64), cand_ids=ids, cand_lp=lp)
