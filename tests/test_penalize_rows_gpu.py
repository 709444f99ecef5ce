"""GPU tests of the penalties (qserve_amd.penalties.penalize_rows, csrc/penalize_rows.hip) and of their place in the engine
(DecodeEngine.set_penalties).  The kernel: the cases of tests/_penalty_cases.py - bit-equality with the float32 restatement, at most one
fp16 ulp from the float64 oracle, everything the rule does not edit bit-identical to the input (canaries in the padding and in neutral
rows), two runs bit-identical.  What each case plants:

    min_vocab    n = 8; n_nodes = 1 without node_tokens; lengths 0, 1, cap and > cap (clamped); prompt_lens 0, = L, > L; the ids -1, n,
                 2^31 - 1 and -2^31 in the history (ignored); scalar parameters
    two_slices   n = 33 000 with row stride 33 008: two slices, the second partial, padding behind n; the ids 0, 32 767, 32 768, n - 1 in the
                 history and on the paths; -1, n itself (node 1 of sequence 2, penalised: a leak would land in the padding's canaries),
                 2^31 - 1 and 2^40 in node_tokens (ignored); a branching tree whose siblings carry different tokens under presence = 50 (a leak from a sibling moves a logit by far more than an ulp); per-sequence
                 parameter tensors with a neutral sequence between two penalised ones; rep > 1 and < 1, negative freq / pres;
                 prompt_lens null; a history length that is no multiple of 4 behind 16-byte loads
    big_vocab    n = 128 256 once, B = 2, n_nodes = 4; history rows with a padded, unaligned stride; L > cap; a per-sequence repetition
                 next to scalar frequency / presence
    chain64      a 64-node chain carrying one token: path multiplicity 63 on a base count of zero and of three; prompt_lens > L
    malformed    parent entries outside 0 .. i - 1 (the node hangs off the root, its children's paths go through it)
    count40000   one id 40 000 times at cap = 40 000: counts above 2^15 in both halves of the count word

All cases contain positive, negative, zero and -inf logits.  The engine tests use the setting of tests/_speculate_engine.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("min_vocab", "two_slices", "big_vocab", "chain64", "malformed", "count40000")


@pytest.fixture(scope="module")
def cases():
    """name -> (case, the float32 restatement's bits): computed once, never changed."""
    from _penalty_cases import gpu_cases, restate32
    return {name: (case, restate32(case)) for name, case in gpu_cases().items()}


def _run(case, gpu):
    """The case through penalties.penalize_rows -> the rows' bits, padding included (uint16 [rows, stride])."""
    from qserve_amd.penalties import penalize_rows
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(gpu)   # noqa: E731
    par = lambda v: dev(v) if isinstance(v, np.ndarray) else v                                # noqa: E731
    store, hist = dev(case["logits"]), dev(case["history"])
    out = penalize_rows(store[:, :case["n"]], hist[:, :case["cap"]], dev(case["lengths"]), dev(case["prompt_lens"]), dev(case["node_tokens"]),
                        None if case["parents"] is None else torch.tensor(case["parents"], dtype=torch.int32, device=gpu),
                        par(case["rep"]), par(case["freq"]), par(case["pres"]))
    assert out.data_ptr() == store.data_ptr()
    torch.cuda.synchronize()
    return store.cpu().numpy().view(np.uint16)


def test_the_cases_are_the_documented_ones(cases):
    assert tuple(cases) == CASES


@pytest.mark.parametrize("name", CASES)
def test_kernel_against_restatement_and_oracle(gpu, cases, name):
    from _penalty_cases import check_against_oracle
    case, want = cases[name]
    got = _run(case, gpu)
    diff = np.argwhere(got != want)
    print(f"{name}: {len(diff)} of {got.size} elements differ from the float32 restatement")
    assert len(diff) == 0, f"{name}: first difference at (row, id) {diff[0].tolist()}: {got[tuple(diff[0])]:#06x} != {want[tuple(diff[0])]:#06x}"
    edited = check_against_oracle(case, got)
    assert edited > 0
    assert np.array_equal(_run(case, gpu), got), f"{name}: two runs differ"


def test_a_history_beyond_the_16_bit_counts_is_refused(gpu):
    """cap = 65 473: QS_EINVAL from the library, through the wrapper's error path; nothing is launched, nothing written."""
    from qserve_amd.penalties import MAX_CAP, penalize_rows
    logits = torch.ones((1, 8), dtype=torch.float16, device=gpu)
    lens = torch.full((1,), 5, dtype=torch.int32, device=gpu)
    with pytest.raises(RuntimeError, match=r"cap=65473.*\(code -1\)"):
        penalize_rows(logits, torch.zeros((1, MAX_CAP + 1), dtype=torch.int32, device=gpu), lens, repetition=2.0)
    assert bool((logits == 1).all())
    penalize_rows(logits, torch.zeros((1, MAX_CAP), dtype=torch.int32, device=gpu), lens, repetition=2.0)    # the largest cap is taken
    assert logits[0].tolist() == [0.5] + [1.0] * 7


# ---- the engine ----------------------------------------------------------------------------------------------------------------------
def test_speculate_penalises_the_rows_the_walk_reads(gpu):
    """Twin engines from one seed and one state, penalties off on A and on on B, one speculate() each: B's last_verify_logits are the
    rule applied to A's - bit-equal to the restatement, within an ulp of the oracle - given A's history, lengths and draft, and B's
    accepted path and bonus token are what the walk gives on the arg-max of those penalised rows."""
    import _accept_engine as E
    import _penalty_engine as PE
    import _speculate_engine as S
    from _penalty_cases import check_against_oracle, restate32
    from _sample_cases import walk
    toks = E.prompt(gpu)
    a, b = S.drafting_engine(toks), PE.penalised_engine(toks)
    assert b.prompt_lens.tolist() == [E.P] * E.B
    hist, lens = a.history.clone(), a.lengths.clone()
    draft = a.draft_tree(E.PAR)
    a.speculate(E.PAR)
    idx, n_acc, am = b.speculate(E.PAR)
    torch.cuda.synchronize()
    case = PE.case_of(a.last_verify_logits, hist, lens, E.P, draft, E.PAR, PE.VALUES)
    got = b.last_verify_logits.reshape(E.B * len(E.PAR), -1).cpu().numpy().view(np.uint16)
    want = restate32(case)
    assert np.array_equal(got, want), f"{int((got != want).sum())} penalised logits differ from the restatement"
    assert int((want != case["logits"].view(np.uint16)).sum()) >= E.B * len(E.PAR) * 20, "the penalty hardly moved the rows"
    check_against_oracle(case, got)
    rows = got.view(np.float16).astype(np.float32).reshape(E.B, len(E.PAR), -1)
    for s in range(E.B):
        best = rows[s].argmax(axis=1)                                   # the first maximum, like the head
        assert am[s].tolist() == best.tolist(), f"sequence {s}: the head's tokens"
        path, bonus = walk(E.PAR, draft[s].tolist(), best.tolist())
        assert idx[s, :int(n_acc[s])].tolist() == path and int(b.tokens[s]) == bonus, f"sequence {s}: the walk"
    assert torch.equal(b.lengths, lens + n_acc)


def test_step_penalises_with_the_text_so_far(gpu):
    """step() on twins: B's token is the arg-max of the rule applied to A's logits under the text before the step.  A negative presence
    lifts the one generated token of the text far above the rest, so the penalty decides the token."""
    import _accept_engine as E
    import _penalty_engine as PE
    import _speculate_engine as S
    from _penalty_cases import restate32
    values = dict(repetition=1.3, frequency=0.0, presence=-30.0)
    toks = E.prompt(gpu)
    a, b = S.drafting_engine(toks), PE.penalised_engine(toks, values)
    hist, lens, first = a.history.clone(), a.lengths.clone(), a.tokens.clone()
    a.step()
    b.step()
    torch.cuda.synchronize()
    logits = torch.matmul(a.final, a.lm_head.t())                       # what A's head read (`final` persists)
    case = PE.case_of(logits.view(E.B, 1, -1), hist, lens, E.P, None, None, values)
    want = restate32(case).view(np.float16).astype(np.float32).argmax(axis=1)
    assert b.tokens.tolist() == want.tolist()
    assert b.tokens.tolist() == first.tolist(), "presence = -30 on the one generated token must make the head repeat it"
    assert torch.equal(b.history[:, E.P + 1], b.tokens.to(torch.int32)) and torch.equal(b.lengths, lens + 1)


def test_penalties_off_is_an_engine_that_never_had_them(gpu):
    import _accept_engine as E
    import _penalty_engine as PE
    import _speculate_engine as S
    toks = E.prompt(gpu)
    a, b = S.drafting_engine(toks), PE.penalised_engine(toks)
    b.set_penalties(None)
    assert b.penalties is None
    for e in (a, b):
        e.speculate(E.PAR)
        e.step()
    E.assert_same_state(a, b, "set_penalties(None)")
    S.assert_same_text(a, b, "set_penalties(None)")
    assert torch.equal(a.last_verify_logits.view(torch.int16), b.last_verify_logits.view(torch.int16))


def test_what_set_penalties_refuses(gpu):
    import _accept_engine as E
    import _penalty_engine as PE
    toks = E.prompt(gpu)
    plain = E.engine(toks)
    with pytest.raises(AssertionError, match="enable_drafting first"):
        plain.set_penalties(1.2)
    e = PE.penalised_engine(toks)
    with pytest.raises(AssertionError, match="repetition=0.0 must be > 0"):
        e.set_penalties(0.0)
    where = [t.data_ptr() for t in e.penalties]
    e.set_penalties(1.1, 0.3, 0.2)
    assert [t.data_ptr() for t in e.penalties] == where and [round(float(t[0]), 4) for t in e.penalties] == [1.1, 0.3, 0.2]
    with pytest.raises(AssertionError, match="device_walk=True"):
        e.verify_tree(torch.zeros((E.B, len(E.PAR)), dtype=torch.int64, device=gpu), E.PAR)
    # every prefill entry refuses before it touches the cache: the engine is still the twin that was never asked
    twin = PE.penalised_engine(toks)
    twin.set_penalties(1.1, 0.3, 0.2)
    for entry, args in ((e.prefill, (E.P, toks)), (e.prefill_chunked, (E.P, 32, toks)),
                        (e.prefill_shared, (toks[:E.P], toks.view(E.B, E.P)[:, :6]))):
        with pytest.raises(AssertionError, match="the prefill head does not penalise"):
            entry(*args)
    E.assert_same_state(e, twin, "a refused prefill")
    e.speculate(E.PAR)
    twin.speculate(E.PAR)
    E.assert_same_state(e, twin, "a round after a refused prefill")


def test_captured_rounds_with_penalties_against_an_eager_twin(gpu):
    """tests/_penalty_engine.py as a program, in a fresh process under a time limit of its own: capture_speculate with penalties on,
    replays against an eager twin, new values through set_penalties after the capture, and a captured step()."""
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tests", "_penalty_engine.py")], cwd=ROOT,
                       capture_output=True, text=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and "PENALTY-CAPTURE-OK" in r.stdout, f"exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
