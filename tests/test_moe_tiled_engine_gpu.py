"""DecodeEngine on TINY_MOE with a prompt pass large enough for the planner to give its grouped GEMMs to the compute-bound tile: B = 4
sequences of 256 tokens are P = 2 048 sorted rows over 4 experts.  Nothing is forced: the engine takes the tile through the plain entries.
Compared with the slow twin of tests/_moe_engine.py (dense GEMM ops per expert) bit for bit: tokens, lengths, last-token states (the
logits are lm_head applied to them) and every K / V pool."""
import pytest
import torch

pytestmark = pytest.mark.gpu
B, L = 4, 256


def _engine(toks, chunk, group_size):
    from qserve_amd.decode import TINY_MOE, DecodeEngine
    e = DecodeEngine(TINY_MOE, batch=B, prompt_len=L, max_new=8, device="cuda:0", seed=5, group_size=group_size)
    e.prefill(L, toks) if chunk is None else e.prefill_chunked(L, chunk, toks)
    return e


@pytest.mark.parametrize("group_size", [-1, 128], ids=["per_chn", "g128"])
def test_prompt_passes_take_the_tile_and_equal_the_slow_twin(gpu, group_size):
    """prefill and prefill_chunked (one chunk of 256: the same P per call) run the tile for gate_up and down and end in the slow twin's
    state; the decode step (P = 8) streams, and one captured step equals the twin's eager one."""
    import _accept_engine as E
    import _moe_engine as M
    from qserve_amd import moe
    from qserve_amd.decode import TINY_MOE
    experts, k, hid, inter = TINY_MOE["experts"], TINY_MOE["experts_per_token"], TINY_MOE["hidden"], TINY_MOE["inter"]
    for N, Kk in ((2 * inter, hid), (hid, inter)):
        assert moe.gemm_form(B * L * k, experts, N, Kk) == "tiled" and moe.gemm_form(B * k, experts, N, Kk) == "streaming"
    forms = []
    original = moe.grouped_gemm
    moe.grouped_gemm = lambda x, xs, xsum, offs, lin, out, **kw: (forms.append(moe.gemm_form(out.size(0), lin.experts, lin.n, lin.k)),
                                                                  original(x, xs, xsum, offs, lin, out, **kw))[1]
    try:
        toks = torch.randint(0, TINY_MOE["vocab"], (B * L,), device=gpu, generator=torch.Generator(device=gpu).manual_seed(1))
        a = _engine(toks, None, group_size)
        assert forms == ["tiled"] * (2 * TINY_MOE["layers"]), forms
        b = M.slow(lambda: _engine(toks, None, group_size))
        E.assert_same_state(a, b, "prefill")
        E.assert_same_state(_engine(toks, L, group_size), b, "prefill_chunked")
        del forms[:]
        a.capture()                                              # (its warm-up is a real step)
        M.slow(b.step)
        E.assert_same_state(a, b, "after capture")
        a.run()
        M.slow(b.step)
        E.assert_same_state(a, b, "captured step")
        assert forms and set(forms) == {"streaming"}, forms
    finally:
        moe.grouped_gemm = original
