"""Engines with set_logprobs on, the comparison of their logs with the float64 oracle of tests/_logprob_cases.py, shared by
tests/test_logprobs_engine_gpu.py - and, run as a program, the bodies of its capture and generate tests (`capture` / `generate` as the
argument).  Those start this file in a fresh Python process because a failed capture leaves the HIP context unusable and
nothing else may share it.

Setting of tests/_speculate_engine.py: TINY, B = 3, P = 70, max_new = 40, seed 5, the 12-node tree PAR, n-gram drafting."""
import os
import sys

import numpy as np
import torch

import _accept_engine as E
import _speculate_engine as S
from _logprob_cases import assert_close, expected_logs, slots

CAP = E.P + 40                                           # the logs' capacity: prompt_len + max_new
SAMPLING = ((0.8, 50, 0.9), dict(seed=3))


def tap(e):
    """Keep the logits every head of `e` hands on (penalised, while on) in e.seen_logits: what the log-probability launch reads."""
    head = e._head

    def tapped(*a, **k):
        e.seen_logits = head(*a, **k)
        return e.seen_logits

    e._head = tapped
    return e


def logs_of(e):
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy().copy() for t in (e.logprob_log, e.rank_log, e.top_ids_log, e.top_lp_log))


def bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def assert_round(before, after, logits, written, T, top, what):
    """`written` (the oracle's slots of the round) hold the oracle's values; every other entry of the logs is bit-equal to `before`."""
    B = before[0].shape[0]
    x = logits.detach().cpu().numpy()
    want = expected_logs(x, written, T, top, B, CAP)
    hit = np.zeros((B, CAP), dtype=bool)
    for b, _, _, _, col in written:
        hit[b, col] = True
    for name, old, new in zip(("lp", "rank", "top_ids", "top_lp"), before, after):
        assert np.array_equal(bits(old)[~hit], bits(new)[~hit]), f"{what}: {name} changed in a column the round does not own"
    assert np.array_equal(after[1][hit], want[1][hit]), f"{what}: ranks differ"
    assert np.array_equal(after[2][hit], want[2][hit]), f"{what}: top ids differ"
    assert_close(after[0][hit], want[0][hit], f"{what} lp")
    assert_close(after[3][hit], want[3][hit], f"{what} top lp")
    return hit


def assert_same_logs(a, b, what):
    for name, x, y in zip(("lp", "rank", "top_ids", "top_lp"), logs_of(a), logs_of(b)):
        assert np.array_equal(bits(x), bits(y)), f"{what}: {name} differs"


def np_(t):
    return t.detach().cpu().numpy()


def capture_main():
    """capture() and capture_speculate() with log-probabilities on (the sampling head on, tempered): every replay leaves state, text and
    all four logs bit-equal to an eager twin's."""
    gpu = torch.device("cuda:0")
    toks = E.prompt(gpu)
    cap, twin, ref = (S.drafting_engine(toks) for _ in range(3))
    for e in (cap, twin, ref):
        e.set_sampling(*SAMPLING[0], **SAMPLING[1])
    for e in (cap, twin):
        e.set_logprobs(top=5, tempered=True)
    cap.capture()                                            # (its warm-up is a real step)
    twin.step()
    ref.step()
    for i in range(3):
        cap.run()
        twin.step()
        ref.step()
        E.assert_same_state(cap, twin, f"captured step {i}")
        S.assert_same_text(cap, twin, f"captured step {i}")
        assert_same_logs(cap, twin, f"captured step {i}")
    lp = logs_of(cap)[0]
    assert np.isfinite(lp[:, E.P + 1:E.P + 5]).all() and np.isnan(lp[:, E.P + 5:]).all() and np.isnan(lp[:, :E.P + 1]).all()
    cap.capture_speculate(E.PAR)
    twin.speculate(E.PAR)
    ref.speculate(E.PAR)
    assert_same_logs(cap, twin, "after capture_speculate")
    ref.set_sampling(None)
    for e in (cap, twin):                                    # the temperature tensor refilled under the graph: greedy, reported at T = 1
        e.set_sampling(1e-6, seed=3)
    S.plant(ref, (cap, twin))
    for i in range(3):
        got = cap.run_speculate()
        want = twin.speculate(E.PAR)
        torch.cuda.synchronize()
        E.assert_same_result(got, want, f"replay {i}")
        E.assert_same_state(cap, twin, f"replay {i}")
        assert_same_logs(cap, twin, f"replay {i}")
        print(f"replay {i}: accepted path lengths {got[1].tolist()}")
        if i == 0:
            assert int(got[1].max()) >= 2, "the planted continuation was accepted nowhere: the replay checked root-only paths"
    lens = cap.lengths.cpu().tolist()
    lp = logs_of(cap)[0]
    for b, L in enumerate(lens):
        assert np.isfinite(lp[b, E.P + 1:L]).all() and np.isnan(lp[b, L:]).all(), f"sequence {b}: the log does not cover its text"
    print("LOGPROB-CAPTURE-OK")


def generate_main():
    """generate() with log-probabilities: a graph captured without the launch is captured again (steps and speculation), and
    logprobs() is aligned with generate()'s texts."""
    from qserve_amd.decode import TINY, DecodeEngine
    gpu = torch.device("cuda:0")
    toks = E.prompt(gpu)
    # -- steps.  (set_logprobs before the prefill: the prefill head records too; tests/test_logprobs_engine_gpu.py checks its entry)
    e = DecodeEngine(TINY, batch=E.B, prompt_len=E.P, max_new=40, device="cuda:0", seed=5)
    e.set_logprobs(top=3)
    e.prefill(E.P, toks)
    e.enable_drafting(toks, **S.NGRAM)
    e.set_logprobs(None)
    e.set_stopping([], [6, 4, 8])
    e.capture()                                              # with the stop launch, without the log-probability launch
    without = e.graph
    e.set_logprobs(top=3)                                    # (clears the logs: the prefill's and the warm-up step's entries are gone)
    texts, reasons, rounds, reads = e.generate(40, poll_every=4)
    assert e.graph is not without, "generate replayed a step graph that holds no log-probability launch"
    assert reasons == [2, 2, 2] and [len(t) for t in texts] == [6, 4, 8]
    out = e.logprobs()
    for b, (text, o) in enumerate(zip(texts, out)):
        assert len(o["logprobs"]) == len(o["ranks"]) == len(o["top_ids"]) == len(o["top_logprobs"]) == len(text)
        # the prefill's token, the first capture()'s warm-up step and the re-capture's: recorded before the logs were cleared, or by a
        # warm-up that ran with the launch - the entries from generate's own first round on must all be there
        first = next(i for i, v in enumerate(o["logprobs"]) if not np.isnan(v))
        assert first <= 2 and all(np.isfinite(v) for v in o["logprobs"][first:]), f"sequence {b}: holes in {o['logprobs']}"
        for i in range(first, len(text)):                    # a greedy head, T = 1, no penalties: every token is its row's first
            assert o["ranks"][i] == 1 and o["top_ids"][i][0] == text[i] and o["top_logprobs"][i][0] == o["logprobs"][i]
            assert o["top_logprobs"][i][0] >= o["top_logprobs"][i][1] >= o["top_logprobs"][i][2]
    with_launch = e.graph
    e.set_logprobs(None)
    e.set_stopping([], [12, 12, 12])
    e.generate(2, poll_every=2)
    assert e.graph is not with_launch, "generate replayed a step graph with the log-probability launch after set_logprobs(None)"
    # -- speculation
    e = S.drafting_engine(toks)
    e.set_stopping([], [9, 9, 9])
    e.capture_speculate(E.PAR)
    without = e.speculate_graph
    e.set_logprobs(top=2)
    texts, reasons, rounds, reads = e.generate(20, parents=E.PAR, poll_every=3)
    assert e.speculate_graph is not without, "generate replayed a speculate graph that holds no log-probability launch"
    again = e.speculate_graph
    e.set_stopping([], [14, 14, 14])
    texts, reasons, rounds, reads = e.generate(20, parents=E.PAR, poll_every=3)
    assert e.speculate_graph is again, "generate captured a matching speculate graph again"
    assert reasons == [2, 2, 2] and [len(t) for t in texts] == [14, 14, 14]
    for text, o in zip(texts, e.logprobs()):
        assert len(o["logprobs"]) == len(text)
        first = next(i for i, v in enumerate(o["logprobs"]) if not np.isnan(v))
        assert first <= 13 and all(o["ranks"][i] == 1 and o["top_ids"][i][0] == text[i] for i in range(first, len(text)))
    print("LOGPROB-GENERATE-OK")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    {"capture": capture_main, "generate": generate_main}[sys.argv[1]]()
