"""DecodeEngine with a table of more than 192 entries (max_len = 12 352): its steps take qs_single_query_attention_long, an engine at
max_len = 12 288 does not, and one captured run equals the eager steps token for token.

Against the existing kernels the per-step ATTENTION OUTPUTS are compared, within TOL, not the tokens: the tiny model's random weights
put greedy candidates within fp16 rounding of each other (measured: sequence 0 of the two engines parts at the second step, 3 against
437, sequence 1 agrees over all 8), so every call of the long entry is repeated through fused_attention.single_query_attention - the
dispatcher's kernel for this table - on the same rows, tables and lengths (both write the same bits into the same slot)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
STEPS, TOL = 8, 2e-3


def _engine(max_len):
    from qserve_amd import decode as D
    eng = D.DecodeEngine(D.TINY, batch=2, prompt_len=70, max_new=max_len - 70, device="cuda:0")
    eng.prefill(70)
    return eng


def test_engine_past_192_pages_takes_the_long_entry(gpu, monkeypatch):
    from qserve_amd import decode as D
    from qserve_amd.plan import attention_long_plan, attention_plan
    entry, errs = D.long_decode.single_query_attention_long, []

    def both(q, k, v, tables, lengths, spt, timestep, base, int4):
        out = entry(q, k, v, tables, lengths, spt, timestep, base, int4)
        ref = D.fused_attention.single_query_attention(q, k, v, tables, lengths, None, 8192, 64, spt, timestep, 128, base, True, int4, True)
        errs.append(float((out.float() - ref.float()).abs().max()))
        return out
    monkeypatch.setattr(D.long_decode, "single_query_attention_long", both)
    ref = _engine(12288)
    ref.step()
    assert not errs, "max_len = 12 288 launches what it launched"
    eng = _engine(12352)
    mb = eng.tables[0].size(-1)
    assert mb > 192 and attention_plan(2, eng.H, eng.Hkv, mb, 12352, eng.int4)["family"] == "valu"
    assert attention_long_plan(2, eng.H, eng.Hkv, mb, eng.int4)["splits"] > 1
    toks = [eng.tokens.clone()]
    for _ in range(STEPS):
        eng.step()
        toks.append(eng.tokens.clone())
    torch.cuda.synchronize()
    print(f"DECODELONG engine: {len(errs)} attention calls, max abs difference to the dispatcher's kernel {max(errs):.3e}")
    assert len(errs) == STEPS * eng.cfg["layers"] and max(errs) <= TOL, errs
    monkeypatch.setattr(D.long_decode, "single_query_attention_long", entry)
    cap = _engine(12352)
    got = [cap.tokens.clone()]
    cap.capture()                          # its warm-up is a real step
    got.append(cap.tokens.clone())
    while len(got) <= STEPS:
        cap.run()
        got.append(cap.tokens.clone())
    torch.cuda.synchronize()
    assert torch.equal(torch.stack(got), torch.stack(toks)), f"captured run differs from the eager steps:\n{torch.stack(got)}\n{torch.stack(toks)}"
