"""DecodeEngine.enable_lora / load_lora / set_lora on the GPU, on the TINY engines of tests/_lora_engine.py (B = 3): every sequence at
-1 against an engine that never heard of LoRA, a mixed batch against three uniform ones row by row, the first lora_rows call of a step
against the float64 oracle, and what refuses.  The capture case runs tests/_lora_engine.py in a fresh process."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def test_every_sequence_at_minus_one_is_the_engine_without_lora(gpu):
    """LoRA on with every id -1 - the four linears on their unfused path, lora_rows launched and leaving at once - against an engine that
    never enabled it: tokens, hidden, lengths and every K / V pool after prefill, prefill_chunked, two step()s, a device-walk verify_tree
    (also its logits and its result) and a speculate() round, bit for bit."""
    import _accept_engine as E
    import _lora_engine as L
    import _speculate_engine as S
    toks = E.prompt(gpu)
    a, b = E.engine(toks), L.lora_engine(toks, [-1, -1, -1])
    assert b._lora and a.lora_table is None and b.lora_ids.tolist() == [-1, -1, -1]
    E.assert_same_state(a, b, "prefill")
    for i in range(2):
        a.step()
        b.step()
        E.assert_same_state(a, b, f"step {i}")
    draft = E.random_draft(np.random.default_rng(7), gpu)
    ra, rb = a.verify_tree(draft, E.PAR, device_walk=True), b.verify_tree(draft, E.PAR, device_walk=True)
    E.assert_same_result(ra, rb, "verify_tree")
    E.assert_same_state(a, b, "verify_tree")
    assert _same_bits(a.last_verify_logits, b.last_verify_logits), "verify_tree: the logits differ"
    a2, b2 = E.engine(toks), L.lora_engine(toks, [-1, -1, -1])       # (fresh: drafting wants the state right behind a prefill)
    for e in (a2, b2):
        e.enable_drafting(toks, **S.NGRAM)
    ra, rb = a2.speculate(E.PAR), b2.speculate(E.PAR)
    E.assert_same_result(ra, rb, "speculate")
    E.assert_same_state(a2, b2, "speculate")
    S.assert_same_text(a2, b2, "speculate")
    assert _same_bits(a2.last_verify_logits, b2.last_verify_logits), "speculate: the logits differ"
    from qserve_amd.decode import TINY, DecodeEngine
    c = DecodeEngine(TINY, batch=E.B, prompt_len=E.P, max_new=40, device="cuda:0", seed=5)
    c.prefill_chunked(E.P, 16, toks)
    E.assert_same_state(c, L.lora_engine(toks, [-1, -1, -1], chunk=16), "prefill_chunked")
    # ... and off again launches what an engine without it launches
    b.set_lora(None)
    assert not b._lora and b._kept_tensors()["lora"] is None
    a.step()
    b.step()
    E.assert_same_state(a, b, "step after set_lora(None)")


def test_a_mixed_batch_gives_every_row_what_its_uniform_batch_gives_it(gpu):
    """Ids [0, 1, -1] against three engines at [0, 0, 0], [1, 1, 1] and [-1, -1, -1]: row b has the bits of row b of the engine at its
    id - after the prefill, a step() and a verify_tree (tokens, hidden, the logits of its nodes, its path).  That rests on every op of
    the stack being row-wise at equal T: the W4A8 GEMMs take exact integer sums per row, the attention and the norms work per
    sequence / row, lora_rows per row.  And the adapters decide something: rows 0 and 1 differ from the base model's."""
    import _accept_engine as E
    import _lora_engine as L
    toks = E.prompt(gpu)
    mixed = L.lora_engine(toks, L.MIXED)
    uniform = [L.lora_engine(toks, [i] * E.B) for i in L.MIXED]
    draft = E.random_draft(np.random.default_rng(9), gpu)

    def rows(what):
        torch.cuda.synchronize()
        for b, u in enumerate(uniform):
            assert int(mixed.tokens[b]) == int(u.tokens[b]) and int(mixed.lengths[b]) == int(u.lengths[b]), f"{what}: row {b} tokens"
            assert _same_bits(mixed.hidden[b], u.hidden[b]), f"{what}: row {b} hidden"

    rows("prefill")
    for e in [mixed] + uniform:
        e.step()
    rows("step")
    res = [e.verify_tree(draft, E.PAR, device_walk=True) for e in [mixed] + uniform]
    rows("verify_tree")
    for b, u in enumerate(uniform):
        assert _same_bits(mixed.last_verify_logits[b], u.last_verify_logits[b]), f"verify_tree: row {b} logits"
        for x, y in zip(res[0], res[1 + b]):
            assert torch.equal(x[b], y[b]), f"verify_tree: row {b} result"
    base = uniform[2]
    for b in (0, 1):
        assert not _same_bits(mixed.last_verify_logits[b], base.last_verify_logits[b]), f"adapter {b} left the logits of the base model"
        assert not _same_bits(mixed.hidden[b], base.hidden[b])
    assert _same_bits(mixed.last_verify_logits[2], base.last_verify_logits[2])


def test_the_first_call_of_a_step_meets_the_oracle(gpu, monkeypatch):
    """The module seam `qserve_amd.lora.lora_rows`, recorded: a step makes 4 calls per layer with rows_per_seq = 1, a 12-node
    verification with 12; the first one - the qkv projection of layer 0, three segments - against the float64 oracle of
    tests/_lora_cases.py under its tolerance, on the engine's own tensors."""
    import _accept_engine as E
    import _lora_cases as K
    import _lora_engine as L
    from qserve_amd import lora as loramod
    toks = E.prompt(gpu)
    e = L.lora_engine(toks, L.MIXED)
    calls, real = [], loramod.lora_rows

    def recording(out, x, x_scale, A, B, scaling, seq_adapter, rows_per_seq, seg_ends, workspace=None):
        rec = dict(before=out.clone(), x=x.clone(), x_scale=x_scale.clone(), A=A, B=B, scaling=scaling, ids=seq_adapter.clone(),
                   rps=rows_per_seq, ends=tuple(seg_ends), ws=workspace)
        real(out, x, x_scale, A, B, scaling, seq_adapter, rows_per_seq, seg_ends, workspace=workspace)
        rec["after"] = out.clone()
        calls.append(rec)
        return out

    monkeypatch.setattr(loramod, "lora_rows", recording)
    e.step()
    torch.cuda.synchronize()
    assert len(calls) == 4 * len(e.layers) and all(c["rps"] == 1 and c["ws"] is e._lora_step_ws for c in calls)
    assert [c["ends"] for c in calls[:4]] == [(512, 768, 1024), (256,), (512, 1024), (256,)]
    c = calls[0]
    assert c["A"] is e.lora_table.layers[0]["qkv"][0] and c["ids"].tolist() == L.MIXED and tuple(c["before"].shape) == (E.B, 1024)
    n = lambda t: t.cpu().numpy()   # noqa: E731
    y, M, active = K.oracle(n(c["before"]), n(c["x"]), n(c["x_scale"]), n(c["A"]), n(c["B"]), n(c["scaling"]), n(c["ids"]), 1, c["ends"])
    got = n(c["after"]).astype(np.float64)
    err, tol = np.abs(got - y), K.tolerance(y, M, 256, L.RANK)
    print(f"max |got - y| / tolerance = {(err / tol).max():.4f}")
    assert active.tolist() == [True, True, False] and (err <= tol).all()
    assert _same_bits(c["after"][2], c["before"][2]) and (n(c["after"])[:2] != n(c["before"])[:2]).mean() > 0.5
    del calls[:]
    e.verify_tree(E.random_draft(np.random.default_rng(2), gpu), E.PAR, device_walk=True)
    assert len(calls) == 4 * len(e.layers) and all(c["rps"] == len(E.PAR) and c["ws"] is not e._lora_step_ws for c in calls)


def test_what_refuses(gpu):
    import _accept_engine as E
    import _lora_engine as L
    from qserve_amd.decode import TINY, DecodeEngine
    toks = E.prompt(gpu)
    e = DecodeEngine(TINY, batch=E.B, prompt_len=E.P, max_new=40, device="cuda:0", seed=5)
    with pytest.raises(AssertionError, match="enable_lora first"):
        e.set_lora([0, 0, 0])
    with pytest.raises(AssertionError, match="enable_lora first"):
        e.load_lora(0, {}, 1.0)
    e.enable_lora(L.SLOTS, L.RANK)
    for bad in ([0, 1], [0.0, 1.0, -1.0], [[0, 1, -1]], 1):
        with pytest.raises(AssertionError, match="one int per sequence"):
            e.set_lora(bad)
    e.set_lora(torch.tensor([1, 0, -1], device=gpu))
    assert e.lora_ids.tolist() == [1, 0, -1] and e.lora_ids.dtype == torch.int32
    prefix, suffix = toks[:64], toks[:E.B * 6].view(E.B, 6)
    with pytest.raises(AssertionError, match="prefill_shared: LoRA is on .* different adapters has different K / V"):
        e.prefill_shared(prefix, suffix)
    e.set_lora(None)
    e.prefill_shared(prefix, suffix)                                   # off again: it runs
    tp = DecodeEngine(TINY, batch=E.B, prompt_len=E.P, max_new=8, device="cuda:0", seed=5, tp_rank=0, tp_world=2)
    with pytest.raises(AssertionError, match="enable_lora: single GPU"):
        tp.enable_lora(L.SLOTS, L.RANK)
    with pytest.raises(AssertionError, match="set_lora: single GPU"):
        tp.set_lora([0, 0, 0])


def test_captured_step_and_round_replay_against_eager_twins(gpu):
    """tests/_lora_engine.py `capture` in a fresh process under a time limit of its own: capture() and capture_speculate with LoRA on,
    three replays each against an eager twin, then other ids filled in place under the captured graphs and one more replay."""
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tests", "_lora_engine.py"), "capture"], cwd=ROOT,
                       capture_output=True, text=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and "LORA-CAPTURE-OK" in r.stdout, f"exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
