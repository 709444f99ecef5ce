"""DecodeEngine with `rope_scaling` in its config (TINY, B = 3, P = 70 - the setting of tests/_accept_engine.py).

Identity: `linear` with factor 1 is a registered profile whose denominators are the base's, bit for bit, so every path that takes the key
- prefill, prefill_chunked, step, verify_tree with the device walk, a captured run - must leave the tokens, lengths and every layer's
pages of an engine without scaling.  Llama3 (original 64: all three bands populated): the agreements between paths that the plain engine's
tests assert hold with the profile on, and the pages differ from the un-scaled engine's."""
import numpy as np
import pytest
import torch

import _accept_engine as AE
from _append_cases import host_pool

pytestmark = pytest.mark.gpu
B, P = AE.B, AE.P
LINEAR1 = dict(rope_type="linear", factor=1.0)
LLAMA3 = dict(rope_type="llama3", factor=8.0, low_freq_factor=1.0, high_freq_factor=4.0, original_max_position_embeddings=64)


def _engine(scaling, max_new=40):
    from qserve_amd.decode import TINY, DecodeEngine
    cfg = dict(TINY, rope_scaling=scaling) if scaling else TINY
    e = DecodeEngine(cfg, batch=B, prompt_len=P, max_new=max_new, device="cuda:0", seed=5)
    assert (e.rope_base < 0) == bool(scaling) and e.cfg["rope_theta"] == TINY["rope_theta"]
    return e


def test_linear_factor_one_is_the_plain_engine(gpu):
    from qserve_amd import rope
    toks, rng = AE.prompt(gpu), np.random.default_rng(3)
    plain, prof = _engine(None), _engine(LINEAR1)
    assert plain.rope_base == 1e4 and rope.profile_state(prof.rope_base)[1] == (P + 40 + 63) // 64 * 64
    assert _engine(LINEAR1).rope_base == prof.rope_base, "the same profile is the same key"
    for e in (plain, prof):
        e.prefill(P, toks)
    AE.assert_same_state(plain, prof, "prefill")
    for i in range(8):
        plain.step(), prof.step()
    AE.assert_same_state(plain, prof, "eight steps")
    ref = _engine(None)
    ref.prefill(P, toks)
    for i in range(8):
        ref.step()
    draft = AE.greedy_draft(ref, rng, gpu)
    got = [e.verify_tree(draft, AE.PAR, device_walk=True) for e in (plain, prof)]
    AE.assert_same_result(got[0], got[1], "verify_tree")
    AE.assert_same_state(plain, prof, "verify_tree")
    assert int(got[0][1].max()) >= 2, "the greedy continuation was accepted nowhere: root-only paths"
    for e in (plain, prof):
        e.capture()
        e.run()
    AE.assert_same_state(plain, prof, "captured run")
    plain.check(), prof.check()
    chunked = [_engine(s, max_new=8) for s in (None, LINEAR1)]
    for e in chunked:
        e.prefill_chunked(P, 48, toks)
    AE.assert_same_state(chunked[0], chunked[1], "prefill_chunked")


def _np(t):
    return t.detach().cpu().numpy()


def test_llama3_profile_paths_agree(gpu):
    from test_append_tree_gpu import ENGINE_MARGIN, _greedy_rule_holds
    toks, rng = AE.prompt(gpu), np.random.default_rng(3)
    # prefill against prefill_chunked (tests/test_append_gpu.py::test_engine_prefill_chunked): layer 0's k / v depend only on per-row
    # deterministic ops (embedding, norm + quant, qkv GEMM, writer)
    whole, chunked, plain = _engine(LLAMA3), _engine(LLAMA3), _engine(None)
    whole.prefill(P, toks), plain.prefill(P, toks)
    chunked.prefill_chunked(P, 48, toks)
    torch.cuda.synchronize()
    assert torch.equal(chunked.pools[0][0], whole.pools[0][0]) and torch.equal(chunked.pools[0][1], whole.pools[0][1]), "layer-0 pages differ"
    assert chunked.lengths.tolist() == whole.lengths.tolist() == [P + 1] * B
    assert bool(((chunked.tokens >= 0) & (chunked.tokens < whole.cfg["vocab"])).all()) and bool(torch.isfinite(chunked.hidden).all())
    assert not torch.equal(whole.pools[0][0], plain.pools[0][0]), "layer-0 K pages equal the un-scaled engine's: the profile was not used"
    assert torch.equal(whole.pools[0][1], plain.pools[0][1]), "layer-0 V pages are not rotated: they equal the un-scaled engine's"
    # step() against a chain draft through verify_tree (tests/test_append_tree_gpu.py::test_engine_verify_tree)
    ref, eng = whole, _engine(LLAMA3)
    eng.prefill(P, toks)
    root, len0 = eng.tokens.clone(), eng.lengths.clone()
    assert torch.equal(ref.tokens, root)
    g, step_logits = [], []
    for _ in range(4):
        ref.step()
        step_logits.append(torch.matmul(ref.final, ref.lm_head.t()).float())
        g.append(ref.tokens.clone())
    n, V = len(AE.PAR), whole.cfg["vocab"]
    draft = torch.from_numpy(rng.integers(0, V, size=(B, n))).to(gpu)
    for k, node in enumerate(AE.CHAIN):
        draft[:, node] = g[k]
        for sib in [c for c in range(n) if AE.PAR[c] == AE.PAR[node] and c != node]:
            draft[:, sib] = (g[k] + 1 + sib) % V
    idx, lens, am = eng.verify_tree(draft, AE.PAR)
    torch.cuda.synchronize()
    idx_h, lens_h, am_h = idx.tolist(), lens.tolist(), am.tolist()
    full = draft.clone()
    full[:, 0] = root
    _greedy_rule_holds(AE.PAR, full.tolist(), idx_h, lens_h, am_h)
    assert torch.equal(eng.lengths, len0 + lens)
    assert eng.tokens.tolist() == [am_h[b][idx_h[b][lens_h[b] - 1]] for b in range(B)]
    vl = eng.last_verify_logits.float()
    diff = max((vl[:, node] - step_logits[k]).abs().max().item() for k, node in enumerate([0] + AE.CHAIN[:3]))
    top2 = torch.stack(step_logits).topk(2, dim=-1).values
    margin = top2[..., 0] - top2[..., 1]
    print(f"llama3 engine: largest logit difference between verify_tree and step() on the same positions {diff:.4e}; "
          f"top-2 margins of the greedy steps min {margin.min().item():.4e}; accepted path lengths {lens_h}")
    for b in range(B):
        for k, node in enumerate(AE.CHAIN):
            if all(margin[j, b].item() > ENGINE_MARGIN for j in range(k + 1)):
                assert lens_h[b] > k + 1 and idx_h[b][k + 1] == node, f"sequence {b}: g_{k + 1} not accepted at a margin {margin[k, b].item():.3e}"
    # layer-0 pages of the slots accepted along the chain: what step() wrote at the same positions
    hp_e = host_pool(_np(eng.pools[0][0]), _np(eng.pools[0][1]), eng.Hkv, True)
    hp_r = host_pool(_np(ref.pools[0][0]), _np(ref.pools[0][1]), ref.Hkv, True)
    tab = (_np(eng.tables[0]) - np.array([eng.pools[0][0].data_ptr(), eng.pools[0][1].data_ptr()])[None, :, None]) // eng.page_bytes
    tab_r = (_np(ref.tables[0]) - np.array([ref.pools[0][0].data_ptr(), ref.pools[0][1].data_ptr()])[None, :, None]) // ref.page_bytes
    assert np.array_equal(tab, tab_r)
    compared = 0
    for b in range(B):
        m = 1      # slots past .. past + m - 1 hold root, g_1 .. g_(m-1); four step()s wrote four slots
        while m < min(lens_h[b], 4) and idx_h[b][m] == AE.CHAIN[m - 1]:
            m += 1
        L = int(len0[b]) - 1 + m
        compared += m
        for which in ("k", "v"):
            for hd in range(eng.Hkv):
                e_ = hp_e.read_tokens(which, tab[b, 0 if which == "k" else 1], hd, L)
                r_ = hp_r.read_tokens(which, tab[b, 0 if which == "k" else 1], hd, L)
                assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(e_, r_)), f"sequence {b}: layer-0 {which} pages differ"
    assert compared > B, "no drafted token was accepted: only root slots were compared"
