"""The penalties without a GPU: the float64 oracle of tests/_penalty_cases.py against the float32 restatement and against an independent
dense formulation, hand-worked contexts, the losslessness of penalised tree verification on a toy model, `qs_penalize_rows`'s argument
validation (which happens before any HIP call), the argument checks of qserve_amd.penalties and its lowering onto the C ABI (through the
host-memory stand-in of tests/_fake_abi.py)."""
import os
import re

import numpy as np
import pytest
import torch

from _penalty_cases import (MALFORMED, check_against_oracle, context, gpu_cases, oracle64, path_nodes, random_case, restate32)
from _sample_cases import Row, depths, philox_uniform, position_keys, walk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _all_cases():
    rng = np.random.default_rng(8)
    return list(gpu_cases().items()) + [(f"random{i}", random_case(rng)) for i in range(300)]


def test_paths_and_contexts_by_hand():
    assert path_nodes([-1, 0, 0, 1, 1, 2, 0], 4) == [1, 4] and path_nodes([-1, 0, 0, 1, 1, 2, 0], 0) == []
    # malformed entries: the node hangs off the root, its children's paths go through it
    assert path_nodes(MALFORMED, 2) == [2] and path_nodes(MALFORMED, 6) == [4, 6] and path_nodes(MALFORMED, 8) == [7, 8]
    case = dict(n=8, n_nodes=3, cap=4, history=np.array([[5, 6, 7, 5, 1]], np.int32), lengths=np.array([9], np.int32),
                prompt_lens=np.array([2], np.int32), node_tokens=np.array([[0, 6, 2]]), parents=[-1, 0, 0])
    assert context(case, 0, 0) == [(5, False), (6, False), (7, True), (5, True)]           # clamped to cap; the root adds nothing
    assert context(case, 0, 2) == context(case, 0, 0) + [(2, True)]                        # never the sibling's 6


def test_the_two_restatements_agree_to_one_fp16_ulp():
    """On every generated case - the GPU tests' and 300 random ones: the float32 restatement against the float64 oracle, and everything
    the rule does not edit untouched."""
    edited = 0
    for name, case in _all_cases():
        try:
            edited += check_against_oracle(case, restate32(case))
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}") from None
    assert edited > 5000


def _dense(case):
    """Counts by np.bincount over each row's context, the HF repetition formula, freq * count + pres * (count > 0), in float64."""
    n, nn = case["n"], case["n_nodes"]
    out = []
    for r in range(case["logits"].shape[0]):
        b, i = divmod(r, nn)
        ctx = context(case, b, i)
        toks = np.array([t for t, _ in ctx if 0 <= t < n], np.int64)
        gens = np.array([t for t, g in ctx if 0 <= t < n and g], np.int64)
        c_all, c_gen = np.bincount(toks, minlength=n), np.bincount(gens, minlength=n)
        rep, freq, pres = (float(np.float32(case[k][b] if isinstance(case[k], np.ndarray) else case[k])) for k in ("rep", "freq", "pres"))
        score = case["logits"][r, :n].astype(np.float64)
        with np.errstate(invalid="ignore"):
            score = np.where(score < 0, score * rep, score / rep)
            score = score - (freq * c_gen + pres * (c_gen > 0))
        out.append((c_all > 0, score))
    return out


def test_oracle_equals_an_independent_dense_formulation():
    for name, case in _all_cases():
        if name in ("big_vocab", "count40000"):              # (the same rule at sizes the loop above makes slow)
            continue
        nn = case["n_nodes"]
        for r, (want, (seen, score)) in enumerate(zip(oracle64(case), _dense(case))):
            b = r // nn
            is_neutral = all(float(np.float32(case[k][b] if isinstance(case[k], np.ndarray) else case[k])) == v
                             for k, v in (("rep", 1.0), ("freq", 0.0), ("pres", 0.0)))
            finite = case["logits"][r, :case["n"]].astype(np.float64) != -np.inf
            assert sorted(want) == ([] if is_neutral else np.nonzero(seen & finite)[0].tolist()), f"{name}: row {r}: edited ids"
            for t, v in want.items():
                assert v == score[t], f"{name}: row {r}: id {t}"


def _toy_logits(prefix, V):
    """A fixed table of logits per prefix: the row is a function of the prefix alone."""
    h = 1469598103934665603
    for t in prefix:
        h = ((h ^ (int(t) + 1)) * 1099511628211) % (1 << 64)
    return (np.random.default_rng(h).standard_normal(V) * 2.0).astype(np.float16)


def _penalised(rows, hist, n_prompt, nodes, par, rep, freq, pres):
    """`rows` fp16 [n_nodes, V] through the rule for ONE sequence whose text is `hist` -> fp16 rows."""
    case = dict(n=rows.shape[1], n_nodes=rows.shape[0], cap=len(hist), history=np.array([hist], np.int32),
                lengths=np.array([len(hist)], np.int32), prompt_lens=np.array([n_prompt], np.int32),
                node_tokens=None if nodes is None else np.array([nodes], np.int64), parents=par, rep=rep, freq=freq, pres=pres,
                logits=rows)
    return restate32(case).view(np.float16)


def test_penalised_tree_verification_is_lossless_on_a_toy_model():
    """Random trees and drafts over an exact toy model, greedy and sampled with position keys: the tokens the walk accepts on the
    PENALISED rows of the tree (node i penalised with the text plus the path to i), plus its bonus token, are the first tokens of the
    chain decoded sequentially with the penalty of the text so far - whatever was drafted.  Drafts repeat tokens of the text and put
    equal tokens on siblings."""
    rng = np.random.default_rng(6)
    V, seed = 12, 77
    longest, moved = 0, 0
    for case in range(500):
        n = int(rng.integers(1, 17))
        par = [-1] + [int(rng.integers(0, i)) for i in range(1, n)]
        dep = depths(par)
        b = int(rng.integers(0, 8))
        ctx = rng.integers(0, V, size=int(rng.integers(1, 8))).tolist()      # the text; its last token is the root's
        n_prompt = int(rng.integers(0, len(ctx) + 1))
        rep, freq, pres = float(rng.choice([1.0, 1.4, 0.7])), float(rng.choice([0.0, 0.6])), float(rng.choice([0.0, 1.0, -0.5]))
        greedy = case % 3 == 0
        T, k, p = (1e-6, 0, 1.0) if greedy else (float(rng.choice([0.7, 1.0])), int(rng.choice([0, 3])), float(rng.choice([0.8, 1.0])))
        L = len(ctx)

        def draw(row, position):
            u = philox_uniform(position_keys([b], [position]), seed)[0]
            return Row(row, T, k, p).token(u)

        # the sequential chain: the token at position L + j follows the text of L + j tokens, penalised with that text (n_nodes = 1)
        chain, text = [], list(ctx)
        for j in range(n + 1):
            raw = _toy_logits(text, V)[None]
            row = _penalised(raw, text, n_prompt, None, None, rep, freq, pres)[0]
            moved += int(not np.array_equal(row.view(np.uint16), raw[0].view(np.uint16)))
            chain.append(draw(row, L + j))
            text.append(chain[-1])
        draft = [ctx[-1]] + rng.integers(0, V, size=n - 1).tolist()
        if n > 1 and case % 2 == 0:                                         # half of the cases: plant the chain along one path
            i = 0
            for j in range(n):
                kids = [c for c in range(n) if par[c] == i]
                if not kids:
                    break
                i = kids[int(rng.integers(0, len(kids)))]
                draft[i] = chain[dep[i] - 1]
                for s in kids:                                              # equal tokens on siblings: the walk takes the lowest
                    if s != i and rng.random() < 0.3:
                        draft[s] = draft[i]
        # the tree: the raw row of node i is the model's on text + path; ONE penalty call edits all rows from the text and the draft
        raw = np.stack([_toy_logits(ctx + [draft[j] for j in path_nodes(par, i)], V) for i in range(n)])
        rows = _penalised(raw, ctx, n_prompt, draft, par, rep, freq, pres)
        sampled = [draw(rows[i], L + dep[i]) for i in range(n)]
        path, bonus = walk(par, draft, sampled)
        got = [draft[i] for i in path[1:]] + [bonus]
        assert got == chain[:len(got)], f"case {case}: walk {got}, chain {chain[:len(got)]}"
        longest = max(longest, len(path))
    assert longest >= 4, "no case accepted a path of depth 3: the walk was only checked near the root"
    assert moved >= 1000, "the penalty hardly ever changed a row: the test compared unpenalised decoding"


def test_the_header_declares_the_entry():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qserve_amd.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+qs_penalize_rows\s*\(", txt)
    assert "65 535" in open(os.path.join(ROOT, "include", "qserve_amd.h")).read()          # the limit of the 16-bit counts is stated


def test_argument_validation_without_gpu(built_lib):
    from qserve_amd._lib import lib

    def call(logits=4096, stride=16, n=16, history=8192, hstride=64, cap=64, lengths=12288, prompt=None, nodes=16384, parents=20480,
             batch=2, n_nodes=4, seq_rep=None):
        return lib.qs_penalize_rows(logits, stride, n, history, hstride, cap, lengths, prompt, nodes, parents, batch, n_nodes, 1.2, 0.1, 0.1,
                                    seq_rep, None, None, None)

    for bad in ("logits", "history", "lengths"):
        assert call(**{bad: None}) == -1 and b"null pointer" in lib.qs_last_error(), bad
    assert call(parents=None) == -1 and b"parents" in lib.qs_last_error()
    assert call(n=7, stride=8) == -1 and b"n=7" in lib.qs_last_error()
    assert call(n=16, stride=20) == -1 and call(n=24, stride=16) == -1
    assert call(n_nodes=0) == -1 and call(n_nodes=65) == -1 and b"n_nodes=65" in lib.qs_last_error()
    assert call(cap=0) == -1 and b"cap=0" in lib.qs_last_error()
    assert call(hstride=63) == -1 and b"hist_stride=63" in lib.qs_last_error()
    assert call(cap=65473, hstride=65473) == -1 and b"cap=65473" in lib.qs_last_error() and b"65535" in lib.qs_last_error()
    assert call(nodes=16388) == -1 and b"8-byte" in lib.qs_last_error()
    assert call(prompt=12290) == -1 and call(seq_rep=12290) == -1 and b"4-byte" in lib.qs_last_error()
    assert call(batch=-1) == -1
    assert call(batch=65536) == -1 and b"batch=65536" in lib.qs_last_error()    # beyond the grid: refused, not a launch failure
    assert call(batch=0) == 0                                                # nothing to do: no launch
    assert call(batch=0, cap=65472, hstride=65472) == 0                      # the largest history the counts can hold


def _host_args():
    logits = torch.zeros((6, 16), dtype=torch.float16)
    hist, lens = torch.zeros((3, 16), dtype=torch.int32), torch.zeros((3,), dtype=torch.int32)
    nodes, par = torch.zeros((3, 2), dtype=torch.int64), torch.tensor([-1, 0], dtype=torch.int32)
    return logits, hist, lens, nodes, par


def test_penalties_argument_checks(built_lib):
    """Wrong dtypes, shapes and values are reported with the argument's name before anything is launched (CPU tensors: the device check
    comes last)."""
    from qserve_amd import penalties as P
    logits, hist, lens, nodes, par = _host_args()
    ok = dict(node_tokens=nodes, parents=par)
    with pytest.raises(RuntimeError, match="logits"):
        P.penalize_rows(logits.float(), hist, lens, **ok)
    with pytest.raises(RuntimeError, match="logits must be"):
        P.penalize_rows(logits[0], hist, lens, **ok)
    with pytest.raises(RuntimeError, match="row stride"):
        P.penalize_rows(torch.zeros((6, 12), dtype=torch.float16), hist, lens, **ok)
    with pytest.raises(RuntimeError, match="n=4"):
        P.penalize_rows(torch.zeros((6, 8), dtype=torch.float16)[:, :4], hist, lens, **ok)
    with pytest.raises(RuntimeError, match="history"):
        P.penalize_rows(logits, hist.long(), lens, **ok)
    with pytest.raises(RuntimeError, match="history must be"):
        P.penalize_rows(logits, hist.t(), lens, **ok)
    with pytest.raises(RuntimeError, match="lengths must be"):
        P.penalize_rows(logits, hist, lens[:2], **ok)
    with pytest.raises(RuntimeError, match="prompt_lens"):
        P.penalize_rows(logits, hist, lens, prompt_lens=lens.long(), **ok)
    with pytest.raises(RuntimeError, match="node_tokens"):
        P.penalize_rows(logits, hist, lens, node_tokens=nodes.int(), parents=par)
    with pytest.raises(RuntimeError, match="node_tokens must be"):
        P.penalize_rows(logits, hist, lens, node_tokens=nodes[:2], parents=par)
    with pytest.raises(RuntimeError, match="needs the tree's parents"):
        P.penalize_rows(logits, hist, lens, node_tokens=nodes)
    with pytest.raises(RuntimeError, match="parents must be"):
        P.penalize_rows(logits, hist, lens, node_tokens=nodes, parents=torch.tensor([-1, 0, 0], dtype=torch.int32))
    with pytest.raises(RuntimeError, match="B \\* n = 3 \\* 2 rows"):
        P.penalize_rows(logits[:3], hist, lens, **ok)
    with pytest.raises(RuntimeError, match="B \\* n = 3 \\* 1 rows"):
        P.penalize_rows(logits, hist, lens)                                  # without node_tokens a sequence has one row
    for bad in (0.0, -1.5, float("nan")):
        with pytest.raises(RuntimeError, match="repetition=.* must be > 0"):
            P.penalize_rows(logits, hist, lens, repetition=bad, **ok)
    with pytest.raises(RuntimeError, match="frequency must be"):
        P.penalize_rows(logits, hist, lens, frequency=torch.zeros((2,)), **ok)
    with pytest.raises(RuntimeError, match="presence"):
        P.penalize_rows(logits, hist, lens, presence=torch.zeros((3,), dtype=torch.float64), **ok)
    with pytest.raises(RuntimeError, match="logits must be on CUDA"):
        P.penalize_rows(logits, hist, lens, **ok)                            # everything else is right: the device is what is left
    assert P.MAX_CAP == 65472


def _fake_penalize_rows(logits, row_stride, n, history, hist_stride, cap, lengths, prompt_lens, node_tokens, parents, batch, n_nodes,
                        rep, freq, pres, seq_rep, seq_freq, seq_pres, stream):
    """qs_penalize_rows over host memory: re-materialise the tensors from the addresses and apply the float32 restatement."""
    import _fake_abi as F
    F.CALLS.append(("qs_penalize_rows", batch, n_nodes, n, cap))
    rows = F._strided_rows(logits, batch * n_nodes, row_stride, row_stride, np.float16)
    par = F._arr(parents, (n_nodes,), np.int32).tolist() if parents else None
    case = dict(n=n, n_nodes=n_nodes, cap=cap, history=F._strided_rows(history, batch, hist_stride, cap, np.int32),
                lengths=F._arr(lengths, (batch,), np.int32), prompt_lens=F._arr(prompt_lens, (batch,), np.int32) if prompt_lens else None,
                node_tokens=F._arr(node_tokens, (batch, n_nodes), np.int64) if node_tokens else None, parents=par,
                rep=F._arr(seq_rep, (batch,), np.float32) if seq_rep else rep, freq=F._arr(seq_freq, (batch,), np.float32) if seq_freq else freq,
                pres=F._arr(seq_pres, (batch,), np.float32) if seq_pres else pres, logits=np.array(rows))
    rows.view(np.uint16)[:] = restate32(case)
    return 0


def test_the_wrapper_lowers_onto_the_abi(built_lib, monkeypatch):
    """qserve_amd.penalties over the host-memory stand-in of the C ABI (tests/_fake_abi.py): strides, the clamp-free hand-over of
    lengths, null pointers for the optional arguments and the scalar-or-tensor convention arrive as the header orders them."""
    import _fake_abi as F
    from qserve_amd import penalties as P
    from qserve_amd._lib import lib
    calls = F.install(monkeypatch)
    monkeypatch.setattr(lib, "qs_penalize_rows", _fake_penalize_rows, raising=True)
    import qserve_amd.backend._util as U
    for attr in ("stream", "expect", "guard"):
        monkeypatch.setattr(P, attr, getattr(U, attr))
    case = gpu_cases()["two_slices"]
    t = lambda a: None if a is None else torch.from_numpy(np.array(a))   # noqa: E731
    store = t(case["logits"])
    logits = store[:, :case["n"]]                                       # a view: the row stride is the padded one
    hist = t(case["history"])
    out = P.penalize_rows(logits, hist, t(case["lengths"]), None, t(case["node_tokens"]), torch.tensor(case["parents"], dtype=torch.int32),
                          t(case["rep"]), t(case["freq"]), t(case["pres"]))
    assert out is logits and calls[-1] == ("qs_penalize_rows", 3, len(case["parents"]), case["n"], case["history"].shape[1])
    assert np.array_equal(store.numpy().view(np.uint16), restate32(case))
    # scalars, prompt_lens, a padded history, n_nodes = 1 without a tree
    case = gpu_cases()["min_vocab"]
    store, wide = t(case["logits"]), torch.zeros((4, 20), dtype=torch.int32)
    wide[:, :16] = t(case["history"])
    P.penalize_rows(store, wide[:, :16], t(case["lengths"]), t(case["prompt_lens"]), repetition=case["rep"], frequency=case["freq"],
                    presence=case["pres"])
    assert calls[-1] == ("qs_penalize_rows", 4, 1, 8, 16)
    assert np.array_equal(store.numpy().view(np.uint16), restate32(case))
    # B == 0 returns at once
    n_calls = len(calls)
    P.penalize_rows(torch.zeros((0, 16), dtype=torch.float16), torch.zeros((0, 16), dtype=torch.int32), torch.zeros((0,), dtype=torch.int32))
    assert len(calls) == n_calls
