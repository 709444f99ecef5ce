"""The prompt LoRA rows under the engine, on the TINY engines of tests/_lora_engine.py (B = 3, adapters [0, 1, -1]): a prefill (70 rows
per sequence: tiles of 64 and 6 rows), a prefill_chunked with chunk 16 (one wave block per tile, a last chunk of 6 rows left to the
planner) and a 16-node verify_tree, with the seam `qserve_amd.lora.rows_form` answering "prompt" for every call of rows_per_seq >= 16,
against the same runs with that seam answering "rows": tokens, lengths, hidden and final rows and every K / V pool, bit for bit.  The
recorded forms say that the first runs did take the prompt kernels."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PAR16 = [-1, 0, 0, 0, 1, 1, 2, 4, 4, 5, 7, 7, 8, 8, 9, 10]


def _run(gpu, monkeypatch, real, form):
    """-> (the engine after prefill + verify_tree, the engine after prefill_chunked, the (rows_per_seq, form) pairs the seam answered)."""
    import _accept_engine as E
    import _lora_engine as L
    from qserve_amd import lora as loramod
    from qserve_amd.decode import TINY
    seen = []

    def rows_form(T, rows_per_seq, slots):
        seen.append((rows_per_seq, form if rows_per_seq >= 16 else real(T, rows_per_seq, slots)))
        return seen[-1][1]

    monkeypatch.setattr(loramod, "rows_form", rows_form)
    toks = E.prompt(gpu)
    e = L.lora_engine(toks, L.MIXED)
    draft = torch.from_numpy(np.random.default_rng(4).integers(0, TINY["vocab"], size=(E.B, len(PAR16)))).to(gpu)
    e.verify_tree(draft, PAR16, device_walk=True)
    c = L.lora_engine(toks, L.MIXED, chunk=16)
    torch.cuda.synchronize()
    return e, c, seen


def test_the_prompt_form_gives_the_bits_of_the_rows_form(gpu, monkeypatch):
    import _accept_engine as E
    from qserve_amd import lora as loramod
    real = loramod.rows_form
    e1, c1, forms = _run(gpu, monkeypatch, real, "prompt")
    per_pass = 4 * len(e1.layers)
    assert {f for f in forms if f[1] == "prompt"} == {(E.P, "prompt"), (len(PAR16), "prompt")}, forms
    assert forms.count((E.P, "prompt")) == per_pass and forms.count((len(PAR16), "prompt")) == per_pass * (1 + E.P // 16), forms
    e0, c0, forms = _run(gpu, monkeypatch, real, "rows")
    assert all(f[1] != "prompt" for f in forms)
    E.assert_same_state(e1, e0, "prefill + verify_tree")
    E.assert_same_state(c1, c0, "prefill_chunked")
    for name, x, y in (("verify_tree logits", e1.last_verify_logits, e0.last_verify_logits), ("final", e1.final, e0.final),
                       ("prefill_chunked final", c1.final, c0.final)):
        assert torch.equal(x.view(torch.int16), y.view(torch.int16)), f"{name} differs between the forms"
