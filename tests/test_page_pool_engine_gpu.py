"""DecodeEngine over a page pool against its static twin (tests/_page_engine.py: TINY, B = 3, P = 125, the same seed): `tokens`,
`lengths`, `hidden` and every row's slots < lengths - 1 of every layer, read through `page_ids` against the twin's own tables, are
byte-identical after prefill, prefill_chunked(16), two steps, a device-walk verify_tree, a speculate round - steps and the 12-node tree
cross slot 128 - and two replays of the captured step (in a process of its own).  A pool one page short starves row 2 at the boundary:
it ends with NO_PAGES, frozen, the other rows stay identical to the twin, the pool's invariant holds, and its text and slots survive
row 0's release and an admit into it."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_a_pooled_engine_is_its_static_twin(gpu):
    import _page_cases as C
    import _page_engine as E
    toks = E.prompt(gpu)
    a, b = E.engine(page_pool=12), E.engine()
    assert a.pager.N == 12 and a.pools[0][0].size(0) == 13 and b.pager is None and b.pools[0][0].size(0) == E.B * b.mb
    C.check_invariant(E.pool_state(a))
    for e in (a, b):
        e.prefill(E.P, toks)
    E.assert_same_rows(a, b, "prefill")
    assert a.pager.owned.tolist() == [2, 2, 2]
    for e in (a, b):
        e.prefill_chunked(E.P, 16, toks)                                     # (a pooled prefill releases every row first)
    E.assert_same_rows(a, b, "prefill_chunked")
    assert a.pager.owned.tolist() == [2, 2, 2] and a.pager.free_pages() == 6
    for e in (a, b):
        e.enable_drafting(toks, **E.NGRAM)
    for i in range(2):
        a.step()
        b.step()
        E.assert_same_rows(a, b, f"step {i}")
    draft = torch.randint(0, 512, (E.B, len(E.PAR)), device=gpu, generator=torch.Generator(device=gpu).manual_seed(3))
    ra, rb = a.verify_tree(draft, E.PAR, device_walk=True), b.verify_tree(draft, E.PAR, device_walk=True)
    for x, y in zip(ra, rb):
        assert torch.equal(x, y)
    E.assert_same_rows(a, b, "verify_tree")
    assert a.pager.owned.tolist() == [3, 3, 3]                              # slots 127 .. 138: the tree crossed into the third page
    for e in (a, b):                                                         # (verify_tree leaves the history to its caller: both
        e.sync_length_bound()                                                # drafters read the same unrecorded columns)
    ra, rb = a.speculate(E.PAR), b.speculate(E.PAR)
    for x, y in zip(ra, rb):
        assert torch.equal(x, y)
    E.assert_same_rows(a, b, "speculate")
    assert torch.equal(a.history, b.history)
    C.check_invariant(E.pool_state(a))
    a.check()


def test_the_captured_step_reserves_at_replay(gpu):
    """tests/_page_engine.py as a program, in a fresh process: capture(), two run() calls that cross into the third page."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_page_engine.py")], cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and "CAPTURE-OK" in r.stdout, f"exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"


def test_a_pool_one_page_short_starves_the_last_row_at_the_boundary(gpu):
    import _page_cases as C
    import _page_engine as E
    from qserve_amd import stopping
    toks = E.prompt(gpu)
    a, b = E.engine(page_pool=8), E.engine()
    for e in (a, b):
        e.prefill(E.P, toks)
        e.enable_drafting(toks, **E.NGRAM)
        e.set_stopping((), E.MAX_NEW)
    for i in range(3):                                                       # slots 125 .. 127: the second page
        a.step()
        b.step()
    E.assert_same_rows(a, b, "before the boundary")
    assert a.finished.tolist() == [0, 0, 0] and a.pager.free_pages() == 2
    frozen = b.history[2, :129].clone()
    for i in range(3):                                                       # slot 128: rows 0 and 1 take the last two pages
        a.step()
        b.step()
    assert a.finished.tolist() == [0, 0, stopping.NO_PAGES] and a.pager.starved.tolist() == [0, 0, 1]
    assert a.pager.owned.tolist() == [3, 3, 2] and a.pager.free_pages() == 0
    assert a.lengths.tolist() == [132, 132, 129] and b.lengths.tolist() == [132, 132, 132]
    E.assert_same_rows(a, b, "behind the boundary", rows=(0, 1))
    assert torch.equal(a.history[:2], b.history[:2]) and torch.equal(a.history[2, :129], frozen) and not a.history[2, 129:].any()
    for li in range(len(a.layers)):                                          # what row 2 wrote since went to the sink: finite (zero scales
        for kv in range(2):                                                  # or quantised K / V), and its own slots < 128 are the twin's
            assert torch.isfinite(a.pools[li][kv][8][-64 * a.Hkv * 4:].view(torch.float16).float()).all()
    x, y = E.row_slots(a, 2, 128), E.row_slots(b, 2, 128)
    assert all(torch.equal(p, q) for p, q in zip(x, y))
    C.check_invariant(E.pool_state(a))
    a.check()                                                                # (the stop rule is on: a starved row is no error)
    # row 0 gives its pages back and takes a new text: what row 2 holds survives the recycling around it
    text2, slots2 = a.history[2].clone(), E.row_slots(a, 2, 128)
    a.pager.release(a.pager.rows_mask([0]))
    assert a.pager.free_pages() == 3 and a.pager.owned.tolist() == [0, 3, 2]
    new = torch.randint(0, 512, (70,), generator=torch.Generator().manual_seed(9))
    a.admit([0], [new], max_new_tokens=8)
    assert a.pager.owned.tolist() == [2, 3, 2] and a.pager.free_pages() == 1
    assert a.finished.tolist() == [0, 0, stopping.NO_PAGES] and a.lengths.tolist() == [71, 132, 129]
    a.step()
    a.step()
    assert a.lengths.tolist() == [73, 134, 129] and a.history[0, :70].tolist() == new.tolist()
    assert torch.equal(a.history[2], text2) and torch.equal(a.history[2, :129], frozen)
    assert all(torch.equal(p, q) for p, q in zip(E.row_slots(a, 2, 128), slots2))
    C.check_invariant(E.pool_state(a))
    a.check()
    a.set_stopping(None)
    with pytest.raises(RuntimeError, match=r"rows \[2\] were refused pages"):
        a.check()
