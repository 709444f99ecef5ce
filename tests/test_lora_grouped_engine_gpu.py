"""The grouped LoRA rows under the engine, on the TINY engines of tests/_lora_engine.py (B = 3, adapters [0, 1, -1]): a step(), a 12-node
verify_tree (tiles that straddle sequences) and an admit of ragged prompts (one adapter id per token) with the form the planner takes
at the seam `qserve_amd.lora.rows_form`, against the same runs with that seam answering "rows": tokens, lengths, hidden and final rows,
the verification's logits and every K / V pool, bit for bit.  The recorded forms say that the first runs did take the grouped kernels."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _run(gpu, monkeypatch, real, form):
    """-> (the engine after step + verify_tree, the engine after a ragged admit, the forms the seam answered during the step).  `form`
    None: the planner `real`; a forced "grouped" leaves calls of rows_per_seq >= 16 (the prompt's prefill), which that form does not
    serve, to the planner."""
    import _accept_engine as E
    import _lora_engine as L
    from qserve_amd import lora as loramod
    from qserve_amd.decode import TINY, DecodeEngine
    seen = []

    def rows_form(T, rows_per_seq, slots):
        planned = form is None or (form == "grouped" and rows_per_seq >= 16)
        seen.append((T, rows_per_seq, real(T, rows_per_seq, slots) if planned else form))
        return seen[-1][2]

    monkeypatch.setattr(loramod, "rows_form", rows_form)
    e = L.lora_engine(E.prompt(gpu), L.MIXED)
    del seen[:]
    e.step()
    step_forms = list(seen)
    e.verify_tree(E.random_draft(np.random.default_rng(4), gpu), E.PAR, device_walk=True)
    a = DecodeEngine(TINY, batch=E.B, prompt_len=130, max_new=40, device="cuda:0", seed=5, page_pool=6)
    a.enable_lora(L.SLOTS, L.RANK)
    L.load_adapters(a)
    a.set_lora(L.MIXED)
    a.enable_drafting(None)
    a.admit([1, 2, 0], [torch.randint(0, 512, (n,), generator=torch.Generator().manual_seed(30 + n)) for n in (40, 9, 23)], chunk=16)
    torch.cuda.synchronize()
    return e, a, step_forms


def test_the_planners_form_gives_the_bits_of_the_rows_form(gpu, monkeypatch):
    import _accept_engine as E
    import _lora_engine as L
    from qserve_amd import lora as loramod
    real = loramod.rows_form
    planned = real(E.B, 1, L.SLOTS)
    # (a planner that keeps "rows" at B = 3 after its measurement: the grouped form is forced through the same seam)
    e1, a1, forms = _run(gpu, monkeypatch, real, None if planned == "grouped" else "grouped")
    assert len(forms) == 4 * len(e1.layers) and all(f == (E.B, 1, "grouped") for f in forms), forms
    e0, a0, forms = _run(gpu, monkeypatch, real, "rows")
    assert all(f == (E.B, 1, "rows") for f in forms)
    E.assert_same_state(e1, e0, "step + verify_tree")
    E.assert_same_state(a1, a0, "admit")
    for name, x, y in (("verify_tree logits", e1.last_verify_logits, e0.last_verify_logits), ("final", e1.final, e0.final),
                       ("admit final", a1.final, a0.final)):
        assert torch.equal(x.view(torch.int16), y.view(torch.int16)), f"{name} differs between the forms"
