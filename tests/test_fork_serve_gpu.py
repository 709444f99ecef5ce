"""DecodeEngine.serve with requests of n = 3 samples on the GPU: six requests through B = 6 rows of a pooled TINY engine
(share_pages=True), length limits only.  tests/_fork_serve.py simulates the loop on the host - the real Scheduler over the restatements
of the counted pool and of the fork - and fixes the two pool sizes: 11 pages, with which samples starve and resume alone, and 40, with
which nothing is preempted.  The first test checks on the CPU that the simulation shows what the GPU run is then held to."""
import pytest

import _fork_serve as S


def _per_request(flat):
    return [flat[3 * i:3 * i + 3] for i in range(len(S.SHAPES))]


def test_the_simulation_preempts_in_the_small_pool_and_saves_pages_in_the_large_one():
    out, stats, st = S.simulate(S.requests(3), S.N_SMALL)
    print(stats, [o["preempted_at"] for o in out])
    assert stats["preempted"] >= 1 and stats["forked"] == 12 and stats["admitted"] == 18 + stats["preempted"] and st["count"] == S.N_SMALL
    assert all(o["reason"] == S.LENGTH and o["length"] == p + m for grp, (p, m) in zip(_per_request(out), S.SHAPES) for o in grp)
    grouped, gstats, _ = S.simulate(S.requests(3), S.N_LARGE)
    single, sstats, _ = S.simulate(S.requests(1), S.N_LARGE)
    assert gstats["preempted"] == sstats["preempted"] == 0 and gstats["peak_pages"] < sstats["peak_pages"]
    assert [o["length"] for o in grouped] == [o["length"] for o in single]


def _engine(pages):
    from qserve_amd.decode import TINY, DecodeEngine
    return DecodeEngine(TINY, batch=S.B, prompt_len=S.CAP_P, max_new=S.MAX_NEW, device="cuda:0", seed=5, page_pool=pages, share_pages=True)


@pytest.mark.gpu
def test_serve_preempts_samples_and_resumes_them_alone(gpu):
    import _page_engine as E
    import _page_ref_cases as R
    from qserve_amd.decode import TINY
    want, want_stats, _ = S.simulate(S.requests(3), S.N_SMALL)
    eng = _engine(S.N_SMALL)
    out, stats = eng.serve(S.requests(3), poll_every=S.POLL, chunk=S.CHUNK)
    print(stats)
    print(want_stats)
    assert len(out) == len(S.SHAPES)
    for i, (res, grp, (p, max_new)) in enumerate(zip(out, _per_request(want), S.SHAPES)):
        assert len(res["samples"]) == 3 and {k: res[k] for k in ("tokens", "reason", "preempted_at")} == res["samples"][0], f"request {i}"
        for smp, w in zip(res["samples"], grp):
            assert smp["reason"] == S.LENGTH and len(smp["tokens"]) == max_new and smp["preempted_at"] == w["preempted_at"], f"request {i}"
            assert all(0 <= t < TINY["vocab"] for t in smp["tokens"])
    assert stats == want_stats and stats["preempted"] >= 1 and stats["forked"] == 12
    state = E.pool_state(eng)
    R.check_invariant(state)
    assert state["owned"].tolist() == [0] * S.B and state["count"] == S.N_SMALL and not state["refs"].any()
    eng.check()


@pytest.mark.gpu
def test_without_preemption_the_samples_are_the_single_requests_texts_on_fewer_pages(gpu):
    _, want_stats, _ = S.simulate(S.requests(3), S.N_LARGE)
    _, want_single, _ = S.simulate(S.requests(1), S.N_LARGE)
    out, stats = _engine(S.N_LARGE).serve(S.requests(3), poll_every=S.POLL, chunk=S.CHUNK)
    single, single_stats = _engine(S.N_LARGE).serve(S.requests(1), poll_every=S.POLL, chunk=S.CHUNK)
    print(stats)
    print(single_stats)
    assert stats == want_stats and single_stats == want_single and stats["preempted"] == single_stats["preempted"] == 0
    assert stats["peak_pages"] < single_stats["peak_pages"]
    assert all("samples" not in r for r in single)
    for i, (res, alone) in enumerate(zip(out, _per_request(single))):
        texts = [s["tokens"] for s in res["samples"]]
        assert texts[0] == texts[1] == texts[2] == res["tokens"], f"request {i}: greedy samples of one prompt differ"
        assert [a["tokens"] for a in alone] == texts, f"request {i}: the samples are not the texts of the same prompts sent alone"
