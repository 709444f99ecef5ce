"""DecodeEngine.score on the GPU: a dense tiny config, TINY_MOE and TINY under two LoRA adapters; B = 3 prompts of P = 70 tokens in
chunks of 32 (three passes, the last one of 6 columns), row 1 a text of 50 tokens right-padded to P.  score must leave the engine where
prefill_chunked leaves a twin, bit for bit, and its lp / greedy must match the float64 scoring of the very rows it handed to
logprobs.score_rows (collected at that seam), under the bound of tests/test_score_rows_gpu.py."""
import pytest
import torch

import _accept_engine as E
import _lora_engine as L

pytestmark = pytest.mark.gpu
CHUNK, LENS = 32, [E.P, 50, E.P]


def engine(kind):
    from qserve_amd.decode import TINY, TINY_MOE, DecodeEngine
    e = DecodeEngine(TINY_MOE if kind == "moe" else TINY, batch=E.B, prompt_len=E.P, max_new=8, device="cuda:0", seed=5)
    if kind == "lora":
        e.enable_lora(L.SLOTS, L.RANK)
        L.load_adapters(e)
        e.set_lora(L.MIXED)
    return e


@pytest.mark.parametrize("kind", ["dense", "moe", "lora"])
def test_score_matches_float64_and_ends_where_prefill_chunked_ends(gpu, monkeypatch, kind):
    from qserve_amd import logprobs
    B, P = E.B, E.P
    toks = E.prompt(gpu)
    a, b = engine(kind), engine(kind)
    seen, real = [], logprobs.score_rows
    monkeypatch.setattr(logprobs, "score_rows", lambda final, *args, **kw: (seen.append(final.clone()), real(final, *args, **kw))[1])
    lp, greedy = a.score(toks.view(B, P), lens=LENS, chunk=CHUNK)
    b.prefill_chunked(P, CHUNK, toks)
    E.assert_same_state(a, b, f"score against prefill_chunked ({kind})")
    assert [f.size(0) for f in seen] == [B * CHUNK, B * CHUNK, B * (P - 2 * CHUNK)]
    assert lp.shape == (B, P) and lp.dtype == torch.float32 and greedy.shape == (B, P) and greedy.dtype == torch.bool

    # the normed row of every (sequence, column), then float64: column p is scored on the row of column p - 1
    final = torch.cat([f.view(B, -1, f.size(1)) for f in seen], dim=1).double().cpu()
    head = a.lm_head.double().cpu()
    x = final[:, :P - 1] @ head.T                                          # [B, P - 1, V]: the logits behind columns 1 .. P - 1
    e = 2.0 * (head.size(1) + 4) * 2.0 ** -24 * (final[:, :P - 1].abs() @ head.abs().T).max(dim=2).values
    t = toks.view(B, P)[:, 1:].cpu()
    want = torch.log_softmax(x, dim=2).gather(2, t.unsqueeze(2)).squeeze(2)
    text = torch.arange(1, P).unsqueeze(0) < torch.tensor(LENS).unsqueeze(1)
    lp, greedy = lp.cpu(), greedy.cpu()
    assert torch.isnan(lp[:, 0]).all() and not greedy[:, 0].any()
    assert torch.isnan(lp[:, 1:][~text]).all() and not greedy[:, 1:][~text].any() and int((~text).sum()) == P - LENS[1]
    err, bound = (lp[:, 1:].double() - want).abs()[text], (2 * e + 1e-5 + 2.0 ** -21 * want.abs())[text]
    print(f"{kind}: max |lp - exact| / bound = {(err / bound).max():.4f}; {int(greedy.sum())} greedy tokens of {int(text.sum())}")
    assert (err <= bound).all()
    top2 = x.topk(2, dim=2).values
    clear = (top2[..., 0] - top2[..., 1] > 2 * (2 * e + 1e-5)) & text
    assert clear.sum() >= 0.9 * text.sum()
    assert torch.equal(greedy[:, 1:][clear], (x.argmax(dim=2) == t)[clear])
