"""DecodeEngine with `sliding_window` on the trace harness of tests/test_engine_trace_cpu.py: windowed entries only, and the refusals."""
import pytest
import torch

from test_engine_trace_cpu import install

W = 64
OTHER_ATTENTION = ("flash_attn_varlen_fwd", "append_attention ", "append_attention_split", "append_attention_shared",
                   "append_tree_attention", "single_query_attention ", "single_query_attention_quant", "single_query_attention_long ")


def _install(monkeypatch):
    """The harness's install, with its device stand-ins also in long_decode (the module no recorded scenario of the harness enters)."""
    import qserve_amd.backend._util as U
    import qserve_amd.long_decode as LD
    D, rec = install(monkeypatch)
    for attr in ("stream", "expect", "guard"):
        monkeypatch.setattr(LD, attr, getattr(U, attr))
    assert D.MISTRAL_7B["sliding_window"] == 4096 and D.DecodeEngine(D.TINY, 2, 5, 4, device="cpu", seed=3).window == 0
    return D, rec


def _engine(D, rec, prompt_len=7):
    return rec.watch(D.DecodeEngine(dict(D.TINY, sliding_window=W), 2, prompt_len, 4, device="cpu", seed=3))


@pytest.mark.parametrize("entry", ["prefill", "prefill_chunked"])
def test_every_attention_is_windowed(built_lib, monkeypatch, entry):
    D, rec = _install(monkeypatch)
    eng = _engine(D, rec)
    eng.prefill(7) if entry == "prefill" else eng.prefill_chunked(7, 3)
    eng.step()
    eng.step()
    appends = [ln.split() for ln in rec.lines if ln.startswith("append_attention_window ")]
    steps = [ln.split() for ln in rec.lines if ln.startswith("single_query_attention_window ")]
    layers, passes = D.TINY["layers"], 1 if entry == "prefill" else 3
    assert len(appends) == passes * layers and len(steps) == 2 * layers, (len(appends), len(steps))
    assert all(a[-2] == str(W) for a in appends), "append entry: window is the argument in front of the stream"
    assert all(s[-3] == str(W) for s in steps), "decode entry: window is the argument in front of num_splits"
    assert not [ln for ln in rec.lines if ln.startswith(OTHER_ATTENTION)], "an attention entry without a window ran"


def test_entries_without_a_windowed_kernel_refuse(built_lib, monkeypatch):
    D, rec = _install(monkeypatch)
    eng = _engine(D, rec, prompt_len=110)
    tokens = torch.randint(0, 512, (2 * 7,), generator=torch.Generator().manual_seed(1))
    eng.prefill_chunked(7, 7, tokens=tokens)
    with pytest.raises(AssertionError, match="sliding_window=64.*append_tree"):
        eng.verify_tree(torch.zeros((2, 3), dtype=torch.int64), [-1, 0, 0])
    with pytest.raises(AssertionError, match="sliding_window=64"):
        eng.enable_drafting(tokens)
    with pytest.raises(AssertionError, match="sliding_window=64.*append_shared"):
        eng.prefill_shared(torch.zeros(70, dtype=torch.int64), torch.zeros((2, 8), dtype=torch.int64))

