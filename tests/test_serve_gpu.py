"""DecodeEngine.serve on the GPU: 8 greedy requests (prompts of 5 to 130 tokens, 6 to 30 new tokens, one stop token - taken from the
middle of a reference text generated without one, so at least one request ends with reason 1) over B = 3 rows of a
pooled TINY engine.  The reference texts come from code that existed before serve: per request a static B = 3 engine with that prompt
in every row - prefill_chunked, enable_drafting, set_stopping, generate - row 0.
  (a) N = 12, nothing starves: every text and reason is the reference's, read_backs <= ceil(rounds / poll_every) + 1, preempted == 0;
  (b) N = 7, the three longest requests first: they take 3 + 2 + 2 pages at admission and would need 9, so rows starve at slot 128 and
      are preempted; every request still completes with reason 1 or 2 and the right length, the invariant holds at the end, requests
      that were never preempted equal the reference, and a preempted one equals it up to its (first) preemption.
The page arithmetic of both scenarios holds for the reference alone: a text of P + m tokens needs ceil((P + m) / 64) pages at most."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B, CAP_P, MAX_NEW, CHUNK, POLL = 3, 130, 40, 48, 4
STOP_FROM = (5, 17)                                                          # the stop token: what request 5 emits as its 18th token without one
REQUESTS = [(130, 20), (125, 30), (120, 25), (5, 6), (70, 12), (33, 30), (64, 9), (100, 15)]     # (prompt tokens, max_new), longest first


def _engine(page_pool=None):
    from qserve_amd.decode import TINY, DecodeEngine
    return DecodeEngine(TINY, batch=B, prompt_len=CAP_P, max_new=MAX_NEW, device="cuda:0", seed=5, page_pool=page_pool)


def _requests():
    g = torch.Generator().manual_seed(17)
    return [(torch.randint(0, 512, (p,), generator=g).tolist(), m) for p, m in REQUESTS]


@pytest.fixture(scope="module")
def reference(gpu):
    """(the stop token, per request (text, reason)): computed once, shared by both scenarios.  The stop token is taken from the middle
    of a text generated WITHOUT one, so that request ends with reason 1 inside a burst - and any other text that holds the token."""
    eng = _engine()

    def texts(stop):
        out = []
        for prompt, max_new in _requests():
            toks = torch.tensor(prompt * B, device=gpu)
            eng.set_stopping(None)
            eng.prefill_chunked(len(prompt), CHUNK, toks)
            eng.enable_drafting(toks)
            eng.set_stopping(stop, max_new)
            text, reasons, _, _ = eng.generate(64, poll_every=POLL)
            assert reasons[0] in (1, 2) and len(text[0]) <= max_new
            out.append((text[0], reasons[0]))
        return out

    free = texts(())
    assert all(reason == 2 and len(text) == m for (text, reason), (_, m) in zip(free, REQUESTS))
    stop = free[STOP_FROM[0]][0][STOP_FROM[1]]
    ref = texts([stop])
    assert ref[STOP_FROM[0]][1] == 1 and len(ref[STOP_FROM[0]][0]) <= STOP_FROM[1] + 1
    return stop, ref


def _complete(res, max_new, stop):
    assert res["reason"] in (1, 2) and 1 <= len(res["tokens"]) <= max_new
    assert len(res["tokens"]) == max_new if res["reason"] == 2 else res["tokens"][-1] == stop
    assert stop not in res["tokens"][:-1]


def test_a_large_pool_serves_every_request_as_the_reference(gpu, reference):
    import _page_cases as C
    import _page_engine as E
    reqs, (STOP, reference) = _requests(), reference
    eng = _engine(page_pool=12)
    out, stats = eng.serve(reqs, stop=[STOP], poll_every=POLL, chunk=CHUNK)
    print(stats, [len(r["tokens"]) for r in out])
    assert len(out) == len(reqs)
    for i, (res, (text, reason)) in enumerate(zip(out, reference)):
        _complete(res, reqs[i][1], STOP)
        assert res["tokens"] == text and res["reason"] == reason and res["preempted_at"] == [], f"request {i}"
    assert out[STOP_FROM[0]]["reason"] == 1
    assert stats["preempted"] == 0 and stats["admitted"] == len(reqs)
    assert stats["read_backs"] <= -(-stats["rounds"] // POLL) + 1
    C.check_invariant(E.pool_state(eng))
    assert eng.pager.free_pages() == 12 and eng.pager.owned.tolist() == [0, 0, 0]
    eng.check()


def test_a_small_pool_preempts_and_still_completes_every_request(gpu, reference):
    import _page_cases as C
    import _page_engine as E
    reqs, (STOP, reference) = _requests(), reference
    eng = _engine(page_pool=7)
    out, stats = eng.serve(reqs, stop=[STOP], poll_every=POLL, chunk=CHUNK)
    print(stats, [(len(r["tokens"]), r["preempted_at"]) for r in out])
    assert stats["preempted"] >= 1 and stats["admitted"] == len(reqs) + stats["preempted"]
    assert sum(len(r["preempted_at"]) for r in out) == stats["preempted"] and any(r["reason"] == 1 for r in out)
    for i, (res, (text, reason)) in enumerate(zip(out, reference)):
        _complete(res, reqs[i][1], STOP)
        if not res["preempted_at"]:
            assert res["tokens"] == text and res["reason"] == reason, f"request {i} (never preempted)"
        else:
            n = res["preempted_at"][0]
            assert n >= 1 and res["tokens"][:n] == text[:n], f"request {i}: its text up to the preemption at {n}"
    C.check_invariant(E.pool_state(eng))
    assert eng.pager.free_pages() == 7
    eng.check()
