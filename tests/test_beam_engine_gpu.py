"""DecodeEngine.set_beams on the GPU (TINY, the setting of tests/_beam_engine.py): W = 1 is greedy decoding; every eager round of
W = 3, G = 2 against the restatement of the selection on the candidates the engine kept, the moved texts, the shared and the copied
pages and the pool's invariant; a forced twin - the same engine with beams off, every row driven along the final hypothesis of the beam
row - whose K / V, hidden rows and summed log-probabilities are the beam engine's bit for bit; a stop token that ends one beam early and
the final ranking; a pool too small for a fork; the captured round against the eager one (a fresh process)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _beam_cases as K
import _beam_engine as S
import _page_engine as E
import _page_ref_cases as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, G, P0, P1 = S.W, S.G, S.P0, S.P1
STEPS = 14


def test_width_1_is_greedy_decoding(gpu):
    prompts = [S.tokens(20 + 7 * r, r) for r in range(3)]
    texts = []
    for width in (1, None):
        e = S.engine(batch=3, width=width)
        for r, X in enumerate(prompts):
            e.admit([r], [X], max_new_tokens=12, chunk=S.CHUNK)
        if width:
            groups, rounds, _ = e.beam_search(16, poll_every=4)
            assert [len(g) for g in groups] == [1, 1, 1]
            texts.append([g[0][0] for g in groups])
            scores = [g[0][1] for g in groups]
            assert all(np.isfinite(s) and s < 0 for s in scores) and [g[0][3] for g in groups] == [2, 2, 2]
            assert not e._beam.moved.any() and e._beam.parent.tolist() == [0, 1, 2]
        else:
            texts.append(e.generate(16, poll_every=4)[0])
        e.check()
    assert texts[0] == texts[1] and all(len(t) == 12 for t in texts[0])


@pytest.fixture(scope="module")
def eager_run(gpu):
    """The eager run of W = 3, G = 2, checked round by round -> (the engine behind STEPS rounds, the prompts)."""
    e = S.engine()
    prompts = S.admit_groups(e)
    B = W * G
    assert e.lengths.tolist() == [P0 + 1] * W + [P1 + 1] * W and bool(torch.isfinite(e.beam_score).all())
    # behind the admit: slot i of a group holds the leader's i-th best first token, scores descending
    sc = e.beam_score.view(G, W).cpu()
    assert bool((sc[:, :-1] >= sc[:, 1:]).all()) and all(len(set(e.tokens[g * W:g * W + W].tolist())) == W for g in range(G))
    two_children = dropped = t_zero = t_pos = 0
    for step in range(STEPS):
        hist, lens, score, toks, fin = (t.cpu().numpy().copy() for t in (e.history, e.lengths, e.beam_score, e.tokens, e.finished))
        ids_before = e.pager.page_ids.cpu().numpy().copy()
        e.step()
        torch.cuda.synchronize()
        bm = e._beam
        parent = bm.parent.cpu().numpy()
        want = K.merge_loop(score, fin, toks, bm.cand_ids.cpu().numpy(), bm.cand_lp.cpu().numpy(), W)
        for key, got in (("parent", parent), ("next_token", bm.next_token.cpu().numpy()), ("cum_out", e.beam_score.cpu().numpy()),
                         ("moved", bm.moved.cpu().numpy()), ("src_rows", bm.src_rows.cpu().numpy())):
            assert np.array_equal(got.view(np.uint8), want[key].view(np.uint8)), f"step {step}: {key} {got} != {want[key]}"
        new_hist, new_lens, ids = e.history.cpu().numpy(), e.lengths.cpu().numpy(), e.pager.page_ids.cpu().numpy()
        assert np.array_equal(e.tokens.cpu().numpy(), want["next_token"])
        for d in range(B):
            p = parent[d]
            L = lens[p]
            assert new_lens[d] == L + 1 and np.array_equal(new_hist[d, :L], hist[p, :L]) and new_hist[d, L] == want["next_token"][d], \
                f"step {step}: row {d} is not its parent's text and the token"
            if p != d:
                w, t = divmod(L, 64)                                         # the fork was told L + 1
                assert np.array_equal(ids[d, :w], ids_before[p, :w]) and np.array_equal(ids[p, :w], ids_before[p, :w]), f"step {step}: shared ids"
                t_zero, t_pos = t_zero + (t == 0), t_pos + (t > 0)
                if t > 0:
                    assert ids[d, w] != ids[p, w] and ids[d, w] >= 0
                    for pair in e.pools:
                        for pool in pair:
                            assert torch.equal(pool[int(ids[d, w])], pool[int(ids[p, w])]), f"step {step}: row {d}'s copied tail page"
        for g in range(G):
            kids = parent[g * W:g * W + W].tolist()
            two_children += any(kids.count(p) >= 2 for p in kids)
            dropped += any(r not in kids for r in range(g * W, g * W + W))
        R.check_invariant(E.pool_state(e))
        e.check()
    assert two_children >= 1 and dropped >= 1, f"seed {S.SEED}: no round with two children of one parent / a dropped row - pick another seed"
    assert t_zero >= 1 and t_pos >= 1, f"moves at t = 0: {t_zero}, at t > 0: {t_pos} - the prompt lengths no longer cross a page boundary"
    return e, prompts


def test_every_eager_round_is_the_restatement_on_the_engines_candidates(eager_run):
    e, _ = eager_run
    assert e.lengths.tolist() == [P0 + 1 + STEPS] * W + [P1 + 1 + STEPS] * W and not e.finished.any()


def test_a_forced_twin_has_the_beams_cache_hidden_rows_and_scores(eager_run):
    """Rests on a row's result not depending on its index or its neighbours (tests/test_fork_engine_gpu.py relies on it too): if only
    this test fails, check that first, with one text in two rows."""
    from qserve_amd.logprobs import logprob_rows
    e, prompts = eager_run
    B = W * G
    starts = [P0] * W + [P1] * W
    lens = e.lengths.tolist()
    text = torch.stack([e.history[b, starts[b]:starts[b] + STEPS + 1] for b in range(B)]).to(torch.int64)   # [B, STEPS + 1] on the device
    slots = [E.row_slots(e, b, lens[b] - 1) for b in range(B)]              # (before the further round below regroups the pages)
    score = e.beam_score.cpu().numpy().copy()
    twin = S.engine(width=None)
    seen, emit = [], twin._emit
    twin._emit = lambda logits, *a, **kw: (seen.append(logits), emit(logits, *a, **kw))[1]
    S.admit_groups(twin, prompts=prompts)
    total = torch.zeros((B,), dtype=torch.float32, device=e.dev)
    rows = torch.arange(B, device=e.dev)
    for i in range(STEPS + 1):
        assert len(seen) == (2 if i == 0 else 1)                           # (the two admits; then one step each)
        for g, logits in enumerate(seen):                                   # an admit's head saw every row: only its group's count
            lp = logprob_rows(logits, text[:, i].contiguous())[0]
            mine = torch.ones_like(lp, dtype=torch.bool) if i else ((rows // W) == g)
            total = torch.where(mine, total + lp, total)                    # one fp32 addition per token, in order
        del seen[:]
        twin.tokens.copy_(text[:, i])
        if i == STEPS:
            break
        twin.step()
    assert np.array_equal(total.cpu().numpy().view(np.uint32), score.view(np.uint32)), f"{total.cpu().numpy()} != {score}"
    assert twin.lengths.tolist() == lens
    for b in range(B):
        for i, (x, y) in enumerate(zip(slots[b], E.row_slots(twin, b, lens[b] - 1))):
            assert torch.equal(x, y), f"row {b}: K / V differ from the forced twin's (piece {i})"
    # `hidden` is the row's own state from before a regroup: one more round on both sides - the beam engine's rows run their final
    # hypotheses' last tokens, whatever it then chooses
    e.step(), twin.step()
    torch.cuda.synchronize()
    assert torch.equal(e.hidden.view(torch.int16), twin.hidden.view(torch.int16))


def test_a_stop_token_freezes_one_beam_and_the_group_is_ranked(gpu):
    from qserve_amd import beams
    dry = S.engine(batch=W)
    X = S.tokens(P0, 1)
    dry.admit([0], [X], max_new_tokens=10, chunk=S.CHUNK, copy_rows=[[1, 2]])
    for _ in range(4):
        dry.step()
    best_first = torch.argsort(dry.beam_score, descending=True).tolist()     # (the best hypothesis' ancestors never left the beam)
    gen = [dry.history[b, P0:P0 + 5].cpu().tolist() for b in best_first]
    early = {t for row in gen for t in row[:3]}
    stop = next((t for row in gen for t in row[3:] if t not in early), None)
    assert stop is not None, f"seed {S.SEED}: no token first emitted in rounds 3 .. 4 - pick another seed"
    e = S.engine(batch=W, stop=[[stop]], length_penalty=0.7)
    e.admit([0], [X], max_new_tokens=10, chunk=S.CHUNK, copy_rows=[[1, 2]])
    groups, rounds, _ = e.beam_search(16, poll_every=4)
    (hyps,) = groups
    fin, lens, cum = e.finished.tolist(), (e.lengths - e.prompt_lens).tolist(), e.beam_score.cpu().tolist()
    assert all(fin) and 1 in fin, f"reasons {fin}: every beam ends, one of them on the stop token"
    for b in range(W):
        if fin[b] == 1:                                                     # frozen with its text and its score
            text = e.history[b, P0:P0 + lens[b]].tolist()
            assert text[-1] == stop and stop not in text[:-1] and lens[b] < 10 and np.isfinite(cum[b])
    scores = [np.float64(cum[b]) / np.float64(max(lens[b], 1)) ** 0.7 for b in range(W)]
    order = sorted((b for b in range(W) if cum[b] != -np.inf), key=lambda b: (-scores[b], b))
    assert [h[0] for h in hyps] == [e.history[b, P0:P0 + lens[b]].tolist() for b in order]
    assert [h[1] for h in hyps] == [cum[b] for b in order] and [h[2] for h in hyps] == [scores[b] for b in order]
    assert [h[3] for h in hyps] == [fin[b] for b in order] and beams.rank(cum, lens, 0.7)[0] == order
    R.check_invariant(E.pool_state(e))
    e.check()


def test_a_pool_too_small_for_a_fork_drops_that_hypothesis(gpu):
    from qserve_amd import stopping
    e = S.engine(batch=W, pages=3)                                          # the leader's two pages and ONE copy of the tail page
    e.admit([0], [S.tokens(70, 1)], max_new_tokens=20, chunk=S.CHUNK, copy_rows=[[1, 2]])
    assert e.finished.tolist() == [0, 0, stopping.NO_PAGES] and e.beam_score[2] == -np.inf and e.pager.free_pages() == 0
    for step in range(5):
        e.step()
        torch.cuda.synchronize()
        # two live rows offer six continuations for three slots: one of them lands in slot 2, whose fork finds no page for the tail
        assert e._beam.moved.tolist()[2] == 1 and e._beam.src_rows.tolist()[2] in (0, 1), f"step {step}"
        assert e.finished.tolist() == [0, 0, stopping.NO_PAGES] and e.beam_score[2] == -np.inf and bool(torch.isfinite(e.beam_score[:2]).all())
        assert e.pager.owned.tolist() == [2, 2, 0] and int(e.pager.error) == 0 and e.lengths.tolist()[:2] == [72 + step] * 2
        R.check_invariant(E.pool_state(e))
    e.check()


def test_the_captured_round_is_the_eager_round(gpu):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_beam_engine.py")], cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and "BEAM-CAPTURE-OK" in r.stdout, f"exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
