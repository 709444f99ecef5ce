"""DecodeEngine.serve under a prefix cache on the GPU: a dozen requests behind a common prefix of 128 tokens, length limits only, over
B = 4 rows of a pooled TINY engine with 10 pages - too few, so rows starve and are preempted.  tests/_prefix_serve.py simulates the
loop on the host (the real Scheduler and PrefixCache over the restatement of the counted pool) and predicts the statistics, which
request is preempted where, and every request's hits; the first test checks on the CPU that the prediction itself shows a preemption,
an eviction and a resumed request that maps its own pages again - and that the same requests starve without the cache too.  The GPU run
must reproduce the prediction.  Generated texts are not compared with an uncached serve: pass shapes differ, and rounding with them."""
import pytest

import _prefix_serve as S


def test_the_simulation_shows_a_preemption_and_a_resumed_hit():
    reqs = S.requests()
    out, stats, (st, cache) = S.simulate(reqs)
    print(stats, [(i, o["preempted_at"], o["hit_tokens"]) for i, o in enumerate(out)])
    assert stats["preempted"] >= 1 and stats["evicted"] >= 1 and stats["admitted"] == len(reqs) + stats["preempted"]
    resumed = [o for o in out if o["preempted_at"]]
    assert resumed and all(len(o["hit_tokens"]) == len(o["preempted_at"]) + 1 for o in out)
    # a resumed request maps its text but the last page - floor((L - 1) / 64) pages, L = P + what it had generated - unless a page
    # of its own was evicted meanwhile; the common prefix never is while a row holds it
    full = [(hit, 64 * ((len(prompt) + at - 1) // 64)) for o, (prompt, _) in zip(out, reqs) for at, hit in zip(o["preempted_at"], o["hit_tokens"][1:])]
    assert all(128 <= hit <= most for hit, most in full) and any(hit == most > 128 for hit, most in full)
    # the first two requests arrive in ONE admit: the second does not see the first's prefix yet; everyone later hits 128 tokens
    assert out[0]["hit_tokens"][0] == out[1]["hit_tokens"][0] == 0 and all(o["hit_tokens"][0] == 128 for o in out[4:])
    assert all(o["reason"] == S.LENGTH and o["length"] == len(p) + m for o, (p, m) in zip(out, reqs))
    assert stats["peak_pages"] <= S.N and stats["hit_tokens"] == sum(sum(o["hit_tokens"]) for o in out)
    _, plain, _ = S.simulate(reqs, prefix_cache=False)
    assert plain["preempted"] >= 1                                          # the pool is too small without the cache as well


@pytest.mark.gpu
def test_serve_reproduces_the_simulation(gpu):
    import _page_ref_cases as R
    import _prefix_engine as E
    from qserve_amd.decode import TINY, DecodeEngine
    reqs = S.requests()
    want, want_stats, _ = S.simulate(reqs)
    eng = DecodeEngine(TINY, batch=S.B, prompt_len=S.CAP_P, max_new=S.MAX_NEW, device="cuda:0", seed=5, page_pool=S.N, prefix_cache=True)
    out, stats = eng.serve(reqs, poll_every=S.POLL, chunk=S.CHUNK)
    print(stats)
    print(want_stats)
    for i, (res, w, (prompt, max_new)) in enumerate(zip(out, want, reqs)):
        assert res["reason"] == S.LENGTH and len(res["tokens"]) == max_new, f"request {i}"
        assert res["preempted_at"] == w["preempted_at"] and res["hit_tokens"] == w["hit_tokens"], f"request {i}"
        assert all(0 <= t < TINY["vocab"] for t in res["tokens"])
    assert any(r["preempted_at"] and r["hit_tokens"][-1] > 0 for r in out)
    assert stats == want_stats
    state = E.pool_state(eng)
    R.check_invariant(state, cache=eng.prefix.by_page)
    assert state["owned"].tolist() == [0] * S.B and eng._row_cached == {}
    eng.evict_prefixes(S.N)
    snap = eng.pager.snapshot()
    assert snap["count"] == S.N and not snap["refs"].any() and len(eng.prefix) == 0
    eng.check()
