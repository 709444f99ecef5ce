"""DecodeEngine.admit on the GPU (TINY, B = 3, the same seed everywhere):
  1. admitting equal-length prompts into every row IS prefill_chunked + enable_drafting - the same calls, so every state tensor and
     every pool byte is identical, over a page pool and without one;
  2. ragged prompts of 5, 70 and 130 tokens in passes of 48: every `append` call against the flash emulation of
     tests/test_append_gpu.py::test_engine_prefill_chunked with its tolerance (4e-3, the project's), layer-0 pages byte-equal to static
     per-length references, lengths = P_r + 1;
  3. an admit into a finished row in the middle of a generation leaves the other rows' tensors unchanged byte for byte, and their
     later texts are those of a twin that admitted nothing;
  4. with sampling, a constraint with per-row start states and top-5 log-probabilities on, the admitted row's first token, state and
     log entry at column P_r are those of a uniform prefill_chunked of that prompt in the same row of a twin;
  5. under set_lora every admitted row runs under its own adapter: a ragged admit against uniform prefill_chunked twins;
  6. while penalties are on the admission head does not penalise: the admitted row against a twin whose penalties are off."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, CAP_P, MAX_NEW = 3, 130, 40


def _engine(page_pool=None):
    from qserve_amd.decode import TINY, DecodeEngine
    return DecodeEngine(TINY, batch=B, prompt_len=CAP_P, max_new=MAX_NEW, device="cuda:0", seed=5, page_pool=page_pool)


def _tokens(n, seed):
    return torch.randint(0, 512, (n,), generator=torch.Generator().manual_seed(seed))


STATE = ("tokens", "lengths", "hidden", "final", "history", "prompt_lens")


@pytest.mark.parametrize("page_pool", [9, None], ids=["pooled", "static"])
def test_a_uniform_admit_is_a_chunked_prefill(gpu, page_pool):
    P = 70
    toks = _tokens(B * P, 1).to(gpu)
    a, b = _engine(page_pool), _engine(page_pool)
    a.prefill_chunked(P, 16, toks)
    a.enable_drafting(toks)
    b.enable_drafting(None)
    b.admit(range(B), list(toks.view(B, P).cpu()), chunk=16)
    torch.cuda.synchronize()
    for k in STATE:
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    for li in range(len(a.layers)):
        for kv in range(2):
            assert torch.equal(a.pools[li][kv], b.pools[li][kv]), f"layer {li} pool {kv}"
    assert a._len_bound == b._len_bound == P + 1 and b._row_starts() == [P] * B
    if page_pool is not None:
        sa, sb = a.pager.snapshot(), b.pager.snapshot()
        for k in ("free", "page_ids", "owned", "starved"):
            assert np.array_equal(sa[k], sb[k]), k
        assert sa["count"] == sb["count"] == 9 - 2 * B and sb["error"] == 0
    b.check()


def test_ragged_prompts_run_through_append_and_fill_their_own_pages(gpu, monkeypatch):
    import _page_engine as E
    import test_append_gpu as TA
    from flash_attn.flash_attn_interface import flash_attn_varlen_func
    from qserve_amd import append as A
    from qserve_amd.decode import TINY
    lens, CH = [5, 70, 130], 48
    H, Hkv, L = TINY["heads"], TINY["kv_heads"], TINY["layers"]
    prompts = [_tokens(n, 20 + n) for n in lens]
    eng = _engine(page_pool=8)
    eng.enable_drafting(None)
    real, calls = A.append, []
    live = {c: [i for i in range(B) if lens[i] > c * CH] for c in range(3)}

    def checked(qkv, cu_seqlens_q, past_lens, kv_pointers, num_heads, num_kv_heads, size_per_token, rope_theta, int4_kv, **kw):
        li, c = len(calls) % L, len(calls) // L
        ns = [min(CH, lens[i] - c * CH) for i in live[c]]                     # a sequence with no token left is not in the pass
        assert past_lens.tolist() == [c * CH] * len(ns) and cu_seqlens_q.tolist() == [0] + np.cumsum(ns).tolist()
        assert torch.equal(kv_pointers, eng.tables[li][live[c]]) and qkv.shape == (sum(ns), eng.qkv_n)
        before = (eng.pools[li][0].clone(), eng.pools[li][1].clone())
        out = real(qkv, cu_seqlens_q, past_lens, kv_pointers, num_heads, num_kv_heads, size_per_token, rope_theta, int4_kv, **kw)
        tab = ((TA._np(kv_pointers) - np.array([eng.pools[li][0].data_ptr(), eng.pools[li][1].data_ptr()])[None, :, None])
               // eng.page_bytes)
        hp = TA.host_pool(TA._np(before[0]), TA._np(before[1]), Hkv, True)
        q, K, V, cu_k = TA.compose(TA._np(qkv), TA._np(cu_seqlens_q), TA._np(past_lens), tab, hp, H, Hkv)
        emu = flash_attn_varlen_func(TA.dev(q), TA.dev(K), TA.dev(V), cu_seqlens_q, TA.dev(cu_k), max(ns), c * CH + max(ns), dropout_p=0.0,
                                     causal=True)
        d = (out.float() - emu.float()).abs().max().item()
        print(f"pass {c} layer {li}: append vs flash emulation {d:.3e}")
        assert d <= 4e-3, f"pass {c} layer {li}: append vs flash emulation {d:.2e}"
        calls.append(d)
        return out

    monkeypatch.setattr(A, "append", checked)
    eng.admit([0, 1, 2], prompts, chunk=CH)
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert len(calls) == L * 3 and eng.lengths.tolist() == [n + 1 for n in lens]
    assert eng.pager.owned.tolist() == [1, 2, 3] and eng.pager.free_pages() == 2
    assert bool(torch.isfinite(eng.hidden).all()) and bool(((eng.tokens >= 0) & (eng.tokens < 512)).all())
    for r, n in enumerate(lens):                                              # layer 0's K / V depend on per-row-deterministic ops only
        ref = _engine()
        ref.prefill(n, prompts[r].repeat(B).to(gpu))
        for i, (x, y) in enumerate(zip(E.row_slots(eng, r, n, layers=[0]), E.row_slots(ref, r, n, layers=[0]))):
            assert torch.equal(x, y), f"row {r} (P = {n}): layer-0 slots differ (piece {i})"
        assert eng.history[r, :n].tolist() == prompts[r].tolist() and int(eng.history[r, n]) == int(eng.tokens[r])
    eng.check()


def test_an_admit_into_a_finished_row_leaves_the_others_alone(gpu):
    import _page_engine as E
    P = 20
    toks = _tokens(B * P, 3).to(gpu)
    a, twin = _engine(page_pool=12), _engine()
    for e in (a, twin):
        e.prefill_chunked(P, 16, toks)
        e.enable_drafting(toks)
        e.set_stopping((), [2, 30, 30])
        for _ in range(3):
            e.step()
    assert a.finished.tolist() == [2, 0, 0] and a.lengths.tolist() == [P + 2, P + 4, P + 4]
    keep = STATE + ("finished", "limit_lens")
    before = {k: getattr(a, k)[1:].clone() for k in keep}
    slots = [E.row_slots(a, r, P + 3) for r in (1, 2)]
    a.admit([0], [_tokens(70, 4)], max_new_tokens=10, chunk=48)
    torch.cuda.synchronize()
    for k in keep:
        assert torch.equal(getattr(a, k)[1:], before[k]), f"rows 1, 2: {k} changed"
    for r, old in zip((1, 2), slots):
        assert all(torch.equal(x, y) for x, y in zip(E.row_slots(a, r, P + 3), old)), f"row {r}: slots changed"
    assert a.finished.tolist() == [0, 0, 0] and a.lengths.tolist() == [71, P + 4, P + 4] and a.limit_lens.tolist() == [80, P + 30, P + 30]
    for _ in range(5):
        a.step()
        twin.step()
    E.assert_same_rows(a, twin, "five steps behind the admit", rows=(1, 2), hidden=False)
    assert torch.equal(a.history[1:], twin.history[1:])
    assert a.lengths.tolist() == [76, P + 9, P + 9] and a.finished.tolist() == [0, 0, 0] and twin.lengths.tolist()[0] == P + 2
    texts, reasons, _, _ = a.generate(12)                                     # texts are cut per row: 70 for row 0, P for the others
    assert reasons[0] == 2 and len(texts[0]) == 10 and texts[0] == a.history[0, 70:80].tolist()
    assert texts[1] == a.history[1, P:int(a.lengths[1])].tolist()
    a.check()


def test_the_first_token_under_features_is_the_prefill_heads(gpu):
    from test_engine_trace_cpu import _dfa
    P, row = 40, 1
    prompt = _tokens(P, 6)
    dfa = _dfa()
    a, twin = _engine(page_pool=6), _engine()
    for e in (a, twin):
        e.set_sampling(0.8, top_k=20, top_p=0.95, seed=11)
        e.set_logprobs(top=5)
        e.set_constraint(dfa, [0, 1, 2])
    twin.prefill_chunked(P, 16, prompt.repeat(B).to(gpu))
    a.enable_drafting(None)
    a.admit([row], [prompt], start_states=[1], chunk=16)
    torch.cuda.synchronize()
    assert int(a.tokens[row]) == int(twin.tokens[row]) and int(a.fsm_state[row]) == int(twin.fsm_state[row])
    assert a.fsm_state.tolist()[0::2] == [0, 2]                               # the other rows' states did not advance
    for k in ("logprob_log", "rank_log", "top_ids_log", "top_lp_log"):
        x, y = getattr(a, k)[row, P], getattr(twin, k)[row, P]
        assert torch.equal(x, y) and not bool(torch.isnan(x.float()).any()), k
    assert bool(torch.isnan(a.logprob_log[0]).all()) and bool(torch.isnan(a.logprob_log[row, :P]).all())
    lp = a.logprobs()                                                         # cut per row: the admitted row's text starts at P
    assert len(lp[row]["logprobs"]) == 1 and lp[row]["top_ids"][0] == a.top_ids_log[row, P].tolist()


def test_an_admit_under_lora_runs_every_row_under_its_own_adapter(gpu):
    """set_lora on, adapters [0, 1, -1]: a ragged admit (40 and 9 tokens in passes of 16 - the short sequence leaves after the first)
    hands lora_rows one adapter id per token; each admitted row's first token, hidden row and pages are those of a uniform
    prefill_chunked of its prompt in the same row of a twin under the same adapters - and not those of the base model."""
    import _lora_engine as LE
    import _page_engine as E
    ids, rows, lens = [0, 1, -1], [1, 2, 0], [40, 9, 23]

    def lora_engine(page_pool=None):
        e = _engine(page_pool)
        e.enable_lora(LE.SLOTS, LE.RANK)
        LE.load_adapters(e)
        e.set_lora(ids)
        return e

    prompts = [_tokens(n, 30 + n) for n in lens]
    a, base = lora_engine(page_pool=6), _engine()
    for e in (a, base):
        e.enable_drafting(None)
        e.admit(rows, prompts, chunk=16)
    torch.cuda.synchronize()
    assert a.lengths.tolist() == [24, 41, 10]
    for r, n, prompt in zip(rows, lens, prompts):
        twin = lora_engine()
        twin.prefill_chunked(n, 16, prompt.repeat(B).to(gpu))
        torch.cuda.synchronize()
        assert int(a.tokens[r]) == int(twin.tokens[r]), f"row {r}: first token"
        assert torch.equal(a.hidden[r].view(torch.int16), twin.hidden[r].view(torch.int16)), f"row {r}: hidden"
        for i, (x, y) in enumerate(zip(E.row_slots(a, r, n), E.row_slots(twin, r, n))):
            assert torch.equal(x, y), f"row {r}: slots differ (piece {i})"
        assert torch.equal(a.hidden[r], base.hidden[r]) == (ids[r] < 0), f"row {r}: adapter {ids[r]} against the base model"
    a.check()


def test_an_admit_while_penalties_are_on_does_not_penalise(gpu, monkeypatch):
    """Two engines in the same mid-generation state, `a` then with set_penalties(1.3, 0.2, 0.2) on: both admit the same 9 tokens (in
    passes of 4) into the finished row 0.  The row's first token, hidden row and pages are equal byte for byte and the admit launches
    no penalize_rows - the step behind it does -; rows 1 and 2 of `a` keep their bytes."""
    import _page_engine as E
    from qserve_amd import penalties
    P, n = 20, 9
    toks, prompt = _tokens(B * P, 3).to(gpu), _tokens(5, 8).repeat(2)[:n]       # (a prompt that repeats itself: penalties would bite)
    a, twin = _engine(page_pool=12), _engine(page_pool=12)
    for e in (a, twin):
        e.prefill_chunked(P, 16, toks)
        e.enable_drafting(toks)
        e.set_stopping((), [2, 30, 30])
        for _ in range(3):
            e.step()
    a.set_penalties(1.3, 0.2, 0.2)
    assert a.finished.tolist() == twin.finished.tolist() == [2, 0, 0]
    keep = STATE + ("finished", "limit_lens")
    before = {k: getattr(a, k)[1:].clone() for k in keep}
    slots = [E.row_slots(a, r, P + 3) for r in (1, 2)]
    real, calls = penalties.penalize_rows, []
    monkeypatch.setattr(penalties, "penalize_rows", lambda *args, **kw: (calls.append(1), real(*args, **kw))[1])
    for e in (a, twin):
        e.admit([0], [prompt], max_new_tokens=10, chunk=4)
    torch.cuda.synchronize()
    assert not calls, "the admission head penalised"
    assert int(a.tokens[0]) == int(twin.tokens[0]) and a.lengths.tolist() == [n + 1, P + 4, P + 4]
    assert torch.equal(a.hidden[0].view(torch.int16), twin.hidden[0].view(torch.int16)), "row 0: hidden"
    for i, (x, y) in enumerate(zip(E.row_slots(a, 0, n), E.row_slots(twin, 0, n))):
        assert torch.equal(x, y), f"row 0: slots differ (piece {i})"
    for k in keep:
        assert torch.equal(getattr(a, k)[1:], before[k]), f"rows 1, 2: {k} changed"
    for r, old in zip((1, 2), slots):
        assert all(torch.equal(x, y) for x, y in zip(E.row_slots(a, r, P + 3), old)), f"row {r}: slots changed"
    a.step()
    assert len(calls) == 1                                                    # (the penalties ARE on: the step's head penalises)
    a.check()
