"""DecodeEngine.admit and the errors of DecodeEngine.serve on the host (the recorder and stubs of tests/test_engine_trace_cpu.py, the page
entries' stand-ins of tests/test_page_pool_contracts.py): what admit launches - a release and ONE reserve with `extra_rows` under a pool,
neither without; the prompts in ragged passes that leave a finished sequence out; one full-batch head - and what it writes per row;
what both refuse before anything runs."""
import numpy as np
import pytest
import torch

import _page_cases as P


def _engine(monkeypatch, page_pool, batch=3):
    import qserve_amd.backend._util as U
    import test_engine_trace_cpu as T
    import test_page_pool_contracts as C
    from qserve_amd import paging
    from qserve_amd._lib import SIGNATURES, lib
    D, rec = T.install(monkeypatch)
    for attr in ("stream", "expect", "guard"):
        monkeypatch.setattr(paging, attr, getattr(U, attr))
    monkeypatch.setattr(lib, "qs_pages_reserve", rec.wrap("qs_pages_reserve", C._fake_reserve, SIGNATURES["qs_pages_reserve"][1]))
    monkeypatch.setattr(lib, "qs_pages_release", rec.wrap("qs_pages_release", C._fake_release, SIGNATURES["qs_pages_release"][1]))
    eng = rec.watch(D.DecodeEngine(D.TINY, batch, 70, 30, device="cpu", seed=3, page_pool=page_pool))
    return eng, rec


def _prompts(lens):
    g = torch.Generator().manual_seed(4)
    return [torch.randint(0, 512, (n,), generator=g) for n in lens]


@pytest.mark.parametrize("page_pool", [5, None], ids=["pooled", "static"])
def test_admit_runs_ragged_passes_and_writes_the_rows_it_was_given(built_lib, monkeypatch, page_pool):
    eng, rec = _engine(monkeypatch, page_pool)
    eng.enable_drafting(None, max_ngram=3, min_match=1, pad_token=7)
    assert eng.lengths.tolist() == [1, 1, 1] and eng.prompt_lens.tolist() == [0, 0, 0] and eng._len_bound == 1
    eng.set_stopping([3], 0)
    prompts = _prompts([3, 70, 9])
    before = {k: getattr(eng, k)[1].clone() for k in ("tokens", "lengths", "hidden", "history", "prompt_lens", "limit_lens", "finished")}
    at = len(rec.lines)
    with np.errstate(all="ignore"):
        eng.admit([2, 0], prompts[:2], max_new_tokens=[5, 8], text_start=[2, 70], chunk=32)
    names = [line.split()[0] for line in rec.lines[at:]]
    if page_pool is None:
        assert "pages_release" not in names and "pages_reserve" not in names
    else:
        assert names[:2] == ["pages_release", "pages_reserve"] and names.count("pages_reserve") == 1 and names.count("pages_release") == 1
        words = rec.lines[at + 1].split()
        assert words[9] == "_all_rows" and words[10] == "tmp" and words[11] == "finished" and words[17] == "0", rec.lines[at + 1]
        snap = eng.pager.snapshot()
        assert snap["owned"].tolist() == [2, 0, 1] and snap["count"] == 2        # served in row order, whatever order `rows` names
        assert snap["page_ids"][0, :2].tolist() == [0, 1] and snap["page_ids"][2, 0] == 2
        P.check_invariant(dict(snap, bases=eng.pager.layer_bases.numpy(), N=5, mb=eng.mb, page_bytes=eng.page_bytes))
    # passes of 32 tokens: (3, 32), (32), (6) rows - the 3-token sequence is left out of the second and third pass
    writers = [line.split() for line in rec.lines[at:] if line.startswith("append_rope_update_kv_cache")]
    assert len(writers) == 3 * len(eng.layers) and names.count("append_attention_split") + names.count("append_attention") == len(writers)
    for k in ("tokens", "lengths", "hidden", "history", "prompt_lens", "limit_lens", "finished"):
        assert torch.equal(getattr(eng, k)[1], before[k]), f"row 1: {k} changed"
    assert eng.lengths.tolist() == [71, 1, 4] and eng.prompt_lens.tolist() == [70, 0, 2] and eng.limit_lens.tolist() == [78, 0, 7]
    assert eng._text_starts == [70, 0, 2] and eng._len_bound == 71
    assert eng.history[2, :3].tolist() == prompts[0].tolist() and eng.history[2, 3] == eng.tokens[2] and not eng.history[2, 4:].any()
    assert eng.history[0, :70].tolist() == prompts[1].tolist() and eng.history[0, 70] == eng.tokens[0]
    assert names[-1] == "stop_update" and rec.lines[-1].split()[-2] == "1"         # the root check


def test_admit_and_serve_refuse_before_anything_runs(built_lib, monkeypatch):
    eng, rec = _engine(monkeypatch, 1)
    with pytest.raises(AssertionError, match="enable_drafting first"):
        eng.admit([0], _prompts([3]))
    eng.enable_drafting(None)
    at = len(rec.lines)
    for match, args, kw in (("distinct row indices", ([0, 0], _prompts([3, 3])), {}),
                            ("distinct row indices", ([3], _prompts([3])), {}),
                            ("one 1-D token sequence per row", ([0, 1], _prompts([3])), {}),
                            ("1 <= P and P", ([0], _prompts([100])), {}),
                            ("1 <= P and P", ([0], [[]]), {}),
                            ("outside the vocabulary", ([0], [[512]]), {}),
                            ("text_start", ([0], _prompts([3])), dict(text_start=4)),
                            ("set_stopping first", ([0], _prompts([3])), dict(max_new_tokens=4)),
                            ("set_constraint first", ([0], _prompts([3])), dict(start_states=1)),
                            ("chunk=0", ([0], _prompts([3])), dict(chunk=0))):
        with pytest.raises(AssertionError, match=match):
            eng.admit(*args, **kw)
    for match, reqs in (("can never fit max_len", [([1] * 60, 41)]),
                        ("can never fit the pool", [([1] * 5, 3), ([1] * 90, 10)]),
                        ("at least one token", [([], 3)])):
        with pytest.raises(AssertionError, match=match):
            eng.serve(reqs)
    assert len(rec.lines) == at and eng.lengths.tolist() == [1, 1, 1] and not eng.history[:, 1:].any() and eng._text_starts is None
