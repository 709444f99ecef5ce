"""DecodeEngine.set_beams on the host (the recorder and stubs of tests/test_engine_trace_cpu.py, the counted page stand-ins of
tests/test_fork_trace_cpu.py, and a steered stand-in of `qs_beam_select` over the row move's restatement): what a beam step launches
and in which order, what set_beams(None) leaves of it (nothing), what a regroup does to the rows and the pool, and the refusals, each
with its reason."""
import numpy as np
import pytest
import torch

import _page_ref_cases as R

STEER = dict(parent=[0, 0, 2], next_token=[5, 6, 7], cum_out=[-1.0, -2.0, -3.0])


def _steered_select(logits, row_stride, n, cum, finished, tokens, batch, width, parent, next_token, cum_out, moved, src_rows, cand_ids, cand_lp,
                    stream):
    """What the entry would write had the group's choice been STEER (the stubbed layers leave no logits to choose from)."""
    import _fake_abi as F
    par = np.asarray(STEER["parent"], np.int32)
    assert batch == par.size and width == 3
    F._arr(parent, (batch,), np.int32)[:] = par
    F._arr(next_token, (batch,), np.int64)[:] = STEER["next_token"]
    F._arr(cum_out, (batch,), np.float32)[:] = STEER["cum_out"]
    F._arr(moved, (batch,), np.int32)[:] = par != np.arange(batch)
    F._arr(src_rows, (batch,), np.int32)[:] = np.where(par != np.arange(batch), par, -1)
    return 0


def _engine(monkeypatch, batch=3, **kw):
    import qserve_amd.backend._util as U
    import test_beam_contracts as BC
    import test_fork_trace_cpu as FT
    from qserve_amd import beams
    from qserve_amd._lib import SIGNATURES, lib
    D, rec, make = FT._engine(monkeypatch, batch, **kw)
    for attr in ("stream", "expect", "guard"):
        monkeypatch.setattr(beams, attr, getattr(U, attr))
    monkeypatch.setattr(lib, "qs_beam_select", rec.wrap("qs_beam_select", _steered_select, SIGNATURES["qs_beam_select"][1]))
    monkeypatch.setattr(lib, "qs_rows_move", rec.wrap("qs_rows_move", BC._fake_move, SIGNATURES["qs_rows_move"][1]))
    return D, rec, make


def _tokens(n, seed):
    return torch.randint(0, 512, (n,), generator=torch.Generator().manual_seed(seed))


def _names(rec, at):
    return [line.split()[0] for line in rec.lines[at:]]


def _state(eng):
    p = eng.pager
    return dict(p.snapshot(), bases=p.layer_bases.numpy(), N=p.N, mb=p.mb, page_bytes=p.page_bytes)


def _admitted(make, beams=None):
    """An engine behind one admit of a prompt of 70 tokens into the group of rows 0, 1, 2."""
    import test_fork_trace_cpu as FT
    eng = FT._ready(make)
    if beams is not None:
        eng.set_beams(beams)
    eng.admit([0], [_tokens(70, 1)], max_new_tokens=8, copy_rows=[[1, 2]])
    return eng


def test_a_beam_step_is_the_greedy_step_with_the_argmax_replaced(built_lib, monkeypatch):
    D, rec, make = _engine(monkeypatch)
    with np.errstate(all="ignore"):
        greedy = _admitted(make)
        at = len(rec.lines)
        greedy.step()
        plain = _names(rec, at)
        eng = _admitted(make, beams=3)
        at = len(rec.lines)
        eng.step()
        beam = _names(rec, at)
    assert plain.count("argmax_rows") == 1
    i = plain.index("argmax_rows")
    assert beam == plain[:i] + ["beam_select", "rows_move", "pages_unhold", "pages_fork"] + plain[i + 1:]
    # what the entries were handed: the engine's persistent tensors, the moved text state in order, the fork with `finished`
    words = {line.split()[0]: line.split() for line in rec.lines[at:]}
    assert words["beam_select"][4:7] == ["beam_score", "finished", "tokens"] and words["beam_select"][7:9] == ["3", "3"]
    assert words["pages_unhold"][11] == words["beam_select"][12] and words["pages_fork"][10] == words["beam_select"][13]
    assert words["pages_fork"][12] == "finished" and words["rows_move"][2] == "3" and words["rows_move"][5] == "5"
    assert [t.data_ptr() for t in eng._beam_moved_tensors()] == [t.data_ptr() for t in (eng.lengths, eng.history, eng.prompt_lens,
                                                                                         eng.limit_lens, eng.finished)]


def test_with_beams_off_the_step_is_the_parents_exactly(built_lib, monkeypatch):
    D, rec, make = _engine(monkeypatch)
    with np.errstate(all="ignore"):
        never = _admitted(make)
        at = len(rec.lines)
        never.step()
        want = rec.lines[at:]
        eng = _admitted(make)
        eng.set_beams(3)
        eng.set_beams(None)
        at = len(rec.lines)
        eng.step()
    assert rec.lines[at:] == want and not any("beam" in line or "rows_move" in line for line in want)
    assert eng._capture_state()["beams"] is None and eng._kept_tensors()["beams"] is None
    eng.set_beams(3)
    assert eng._capture_state()["beams"] == 3 and len(eng._kept_tensors()["beams"]) == 9


def test_a_regroup_moves_the_text_and_the_pages(built_lib, monkeypatch):
    D, rec, make = _engine(monkeypatch)
    with np.errstate(all="ignore"):
        eng = _admitted(make, beams=3)
        eng.history[1, 3] = 99                                              # row 1 differs: the regroup must overwrite it
        eng.limit_lens[1] = 75
        before = _state(eng)
        hist0 = eng.history[0].clone()
        eng.step()
    snap = eng.pager.snapshot()
    assert snap["error"] == 0 and not snap["starved"].any()
    R.check_invariant(_state(eng))
    assert eng.tokens.tolist() == STEER["next_token"] and eng.beam_score.tolist() == STEER["cum_out"]
    assert torch.equal(eng.history[1], hist0) and eng.limit_lens.tolist() == [78, 78, 78] and eng.lengths.tolist()[1] == eng.lengths.tolist()[0]
    # the text of 71 tokens wrote slot 70; the fork was told 72: page 0 shared, page 1 (7 slots) copied into a page of row 1's own
    assert snap["page_ids"][1, 0] == snap["page_ids"][0, 0] == before["page_ids"][0, 0] and snap["refs"][snap["page_ids"][0, 0]] == 3
    assert snap["page_ids"][1, 1] not in (snap["page_ids"][0, 1], snap["page_ids"][2, 1]) and snap["owned"].tolist() == [2, 2, 2]
    k0, _ = eng.pools[0]
    assert torch.equal(k0[snap["page_ids"][1, 1]], k0[snap["page_ids"][0, 1]])
    assert np.array_equal(snap["page_ids"][[0, 2]], before["page_ids"][[0, 2]])   # the rows that stay keep their pages
    eng.pager.check(starved=True)


def test_admit_under_beams_takes_whole_groups(built_lib, monkeypatch):
    D, rec, make = _engine(monkeypatch, batch=6)
    import test_fork_trace_cpu as FT
    with np.errstate(all="ignore"):
        eng = FT._ready(make)
        eng.set_beams(3)
        at = len(rec.lines)
        for rows, copies in (([0], None), ([0], [[1]]), ([1], [[2, 3]]), ([0], [[2, 1]]), ([3], [[4, 5, 0]]), ([0, 3], [[1, 2], [5, 4]])):
            with pytest.raises(AssertionError, match="every prompt starts one whole group"):
                eng.admit(rows, [_tokens(20, 1)] * len(rows), max_new_tokens=4, copy_rows=copies)
        assert len(rec.lines) == at
        monkeypatch.setitem(STEER, "parent", [0, 0, 0, 3, 3, 3])
        monkeypatch.setitem(STEER, "next_token", [5, 6, 7, 8, 9, 10])
        monkeypatch.setitem(STEER, "cum_out", [-1.0, -2.0, -3.0, -4.0, -5.0, -6.0])
        eng.admit([3], [_tokens(20, 1)], max_new_tokens=4, copy_rows=[[4, 5]])
    names = _names(rec, at)
    assert names.count("beam_select") == 1 and "argmax_rows" not in names and "rows_move" not in names
    assert eng.tokens.tolist()[3:] == [8, 9, 10] and eng.beam_score.tolist() == [0.0, 0.0, 0.0, -4.0, -5.0, -6.0]
    assert eng.history[3:, 20].tolist() == [8, 9, 10] and eng.lengths.tolist()[3:] == [21] * 3


def test_every_refusal_raises_with_its_reason(built_lib, monkeypatch):
    D, rec, make = _engine(monkeypatch)
    import test_fork_trace_cpu as FT
    with np.errstate(all="ignore"):
        # what set_beams asks for
        with pytest.raises(AssertionError, match="single GPU, with the lm_head"):
            D.DecodeEngine(D.TINY, 4, 200, 30, device="cpu", seed=3, tp_rank=0, tp_world=2).set_beams(2)
        plain = D.DecodeEngine(D.TINY, 3, 200, 30, device="cpu", seed=3, page_pool=9)
        plain.enable_drafting(None)
        with pytest.raises(AssertionError, match="counted page pool"):
            plain.set_beams(3)
        static = D.DecodeEngine(D.TINY, 3, 200, 30, device="cpu", seed=3)
        with pytest.raises(AssertionError, match="counted page pool"):
            static.set_beams(3)
        cached = FT._engine(monkeypatch, prefix_cache=True)[2]()
        cached.enable_drafting(None)
        cached.set_stopping((), 0)
        with pytest.raises(AssertionError, match="cannot follow a regroup"):
            cached.set_beams(3)
        raw = make()
        with pytest.raises(AssertionError, match="enable_drafting first"):
            raw.set_beams(3)
        eng = FT._ready(make, stopping=False)
        with pytest.raises(AssertionError, match="set_stopping first"):
            eng.set_beams(3)
        eng.set_stopping((), 0)
        for width in (0, 2, 33):
            with pytest.raises(AssertionError, match=f"width={width} .* must divide the batch of 3 rows"):
                eng.set_beams(width)
        eng.set_sampling(0.8, seed=1)
        with pytest.raises(AssertionError, match="sampling is on"):
            eng.set_beams(3)
        eng.set_sampling(None)
        eng.set_logprobs(2)
        with pytest.raises(AssertionError, match="set_logprobs is on"):
            eng.set_beams(3)
        eng.set_logprobs(None)
        eng.set_beams(3, length_penalty=0.5)
        assert eng.beams == 3 and eng._beam_penalty == 0.5
        eng.admit([0], [_tokens(20, 1)], max_new_tokens=4, copy_rows=[[1, 2]])
    # what refuses while beams are on - before any call
    at = len(rec.lines)
    PAR = [-1, 0, 0]
    for match, call in (("set_sampling: beam search is on .* chosen by score, not drawn", lambda: eng.set_sampling(0.8)),
                        ("set_logprobs: beam search is on .* do not follow a regroup", lambda: eng.set_logprobs(2)),
                        ("fork: beam search is on .* the round itself decides", lambda: eng.fork(0, [1])),
                        ("serve: beam search is on .* lives and ends as a whole", lambda: eng.serve([(_tokens(5, 1), 2)])),
                        ("prefill: beam search is on .* chosen by admit", lambda: eng.prefill(5)),
                        ("prefill_chunked: beam search is on", lambda: eng.prefill_chunked(5, 2)),
                        ("prefill_shared: beam search is on", lambda: eng.prefill_shared(_tokens(70, 1), torch.zeros((3, 4), dtype=torch.int64))),
                        ("verify_tree: beam search is on .* one path per row",
                         lambda: eng.verify_tree(torch.zeros((3, 3), dtype=torch.int64), PAR, device_walk=True)),
                        ("capture_verify: beam search is on", lambda: eng.capture_verify(PAR)),
                        ("speculate: beam search is on", lambda: eng.speculate(PAR)),
                        ("capture_speculate: beam search is on", lambda: eng.capture_speculate(PAR)),
                        ("generate: beam search is on", lambda: eng.generate(4, parents=PAR))):
        with pytest.raises(AssertionError, match=match):
            call()
    assert len(rec.lines) == at
    with pytest.raises(AssertionError, match="beam_search: set_beams first"):
        FT._ready(make).beam_search(4)
    # set_sampling(None) / set_logprobs(None) stay allowed, and set_beams(None) lifts every refusal
    eng.set_sampling(None)
    eng.set_logprobs(None)
    eng.set_beams(None)
    eng.set_logprobs(1)
    eng.set_logprobs(None)
