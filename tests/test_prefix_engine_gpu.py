"""DecodeEngine(prefix_cache=True) on the GPU (tests/_prefix_engine.py: TINY, B = 3, 12 pages): a prompt that maps the cached pages of
an earlier one against a pooled twin that computes it whole.  Bit-identity is asked only where the construction gives identical
launches: the twin admits Y in chunks of 128, so its second pass - 61 tokens at past 128 over pages that are byte-equal to the cached
ones, which the same first pass wrote - is the one pass the cached admit runs.  `tokens`, `hidden`, `lengths` and every slot
< lengths - 1 of that row are equal byte for byte behind the admit and behind each of four steps, the fourth across a page boundary;
then: releasing the other holder, a tree verification and a speculation round leave the shared pages' bytes alone; the captured step
replays across a page boundary (a fresh process); releasing everything and evicting frees every page; a prompt of exactly 128 cached
tokens maps one page, not two."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _freeze(eng, row):
    """What serve does to a harvested row: a one-token text at its limit, frozen."""
    from qserve_amd import stopping
    eng.lengths[row], eng.finished[row] = 1, stopping.LENGTH


def test_a_cached_admit_is_the_twins_second_pass_and_the_steps_stay_equal(gpu):
    import _page_engine as E
    import _page_ref_cases as R
    import _prefix_engine as S
    a, twin = S.pair()
    E.assert_same_rows(a, twin, "admit", rows=[1])
    snap = a.pager.snapshot()
    shared = snap["page_ids"][0, :2].tolist()
    assert snap["owned"].tolist() == [3, 3, 0] and snap["page_ids"][1, :2].tolist() == shared
    assert snap["refs"][shared].tolist() == [3, 3] and snap["count"] == S.N - 4 and sorted(a.prefix.by_page) == sorted(shared)
    assert a._row_cached == {0: shared, 1: shared} and a.lengths.tolist() == [151, 190, 1]
    R.check_invariant(S.pool_state(a), cache=shared)
    before = S.page_bytes(a, shared)
    for i in range(4):
        a.step()
        twin.step()
        E.assert_same_rows(a, twin, f"step {i}", rows=[1])
    assert a.pager.owned.tolist() == [3, 4, 0] and a.lengths.tolist() == [155, 194, 1]
    # the other holder lets go: the row steps on, the shared pages keep their bytes and two holders
    _freeze(a, 0)
    a.release_rows([0])
    assert a.pager.refs[shared].tolist() == [2, 2] and a.pager.free_pages() == S.N - 4 - 1 + 1 and a._row_cached == {1: shared}
    for i in range(2):
        a.step()
        twin.step()
        E.assert_same_rows(a, twin, f"step {i} behind the release", rows=[1])
    assert all(torch.equal(x, y) for x, y in zip(before, S.page_bytes(a, shared)))
    R.check_invariant(S.pool_state(a), cache=shared)
    a.check()


def test_tree_rounds_leave_the_shared_pages_alone(gpu):
    import _page_engine as E
    import _page_ref_cases as R
    import _prefix_engine as S
    a, _ = S.pair()
    shared = a.pager.page_ids[1, :2].tolist()
    before = S.page_bytes(a, shared)
    draft = torch.randint(0, 512, (S.B, len(E.PAR)), device=gpu, generator=torch.Generator(device=gpu).manual_seed(3))
    a.verify_tree(draft, E.PAR, device_walk=True)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(before, S.page_bytes(a, shared))), "verify_tree wrote a shared page"
    R.check_invariant(S.pool_state(a), cache=shared)
    a.sync_length_bound()
    a.speculate(E.PAR)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(before, S.page_bytes(a, shared))), "speculate wrote a shared page"
    R.check_invariant(S.pool_state(a), cache=shared)
    assert a.pager.refs[shared].tolist() == [3, 3]
    a.check()


def test_the_captured_step_of_a_counted_engine_replays_across_a_page_boundary(gpu):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_prefix_engine.py")], cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and "PREFIX-CAPTURE-OK" in r.stdout, f"exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"


def test_releasing_everything_and_evicting_frees_every_page(gpu):
    import _page_ref_cases as R
    import _prefix_engine as S
    a, _ = S.pair()
    shared = a.pager.page_ids[1, :2].tolist()
    for r in (0, 1):
        _freeze(a, r)
    a.release_rows([0, 1])
    assert a.pager.free_pages() == S.N - 2 and a.prefix.evictable() == 2 and a._row_cached == {}
    R.check_invariant(S.pool_state(a), cache=shared)
    assert sorted(a.evict_prefixes(5)) == sorted(shared) and len(a.prefix) == 0
    snap = a.pager.snapshot()
    assert snap["count"] == S.N and not snap["refs"].any() and snap["error"] == 0
    R.check_invariant(S.pool_state(a))


def test_a_prompt_of_exactly_128_cached_tokens_maps_one_page(gpu):
    """Its last token is recomputed - the head needs its hidden row -, so the second page is the row's own."""
    import _page_ref_cases as R
    import _prefix_engine as S
    a = S.engine(True)
    a.admit([0], [S.X], max_new_tokens=8, chunk=S.CHUNK)
    a.admit([2], [S.X[:128]], max_new_tokens=8, chunk=S.CHUNK)
    snap = a.pager.snapshot()
    shared = snap["page_ids"][0, :2].tolist()
    assert snap["owned"].tolist() == [3, 0, 2]                              # slots 0 .. 127: the cached page and one of its own
    assert snap["page_ids"][2, 0] == shared[0] and snap["page_ids"][2, 1] not in shared
    assert snap["refs"][shared].tolist() == [3, 2] and a._row_cached == {0: shared, 2: shared[:1]}
    R.check_invariant(S.pool_state(a), cache=shared)
    assert a.lengths.tolist() == [151, 1, 129]
    a.check()


def test_refusals(gpu):
    from qserve_amd.decode import TINY, DecodeEngine
    with pytest.raises(AssertionError, match="give page_pool=N"):
        DecodeEngine(TINY, batch=2, prompt_len=8, max_new=8, device="cuda:0", prefix_cache=True)
