"""The setting of tests/test_beam_engine_gpu.py - TINY, groups of W = 3 rows over a counted pool - and, run as a program, the body of
its capture test: ten rounds of a captured beam step against ten eager ones of an identical engine.  That test starts this file in a
fresh Python process for the reason tests/_page_engine.py gives: a failed capture leaves the HIP context unusable.  The helpers of
tests/_page_engine.py are used read-only."""
import os
import sys

import torch

W, G, CAP_P, MAX_NEW, N, CHUNK = 3, 2, 150, 40, 24, 128
SEED = 5          # the engine's weights: the eager test asserts that its run holds a parent with two children and a dropped row
P0, P1 = 62, 130  # the groups' prompt lengths: 14 steps behind 62 cross slot 64 into a second page; t = 0 and t > 0 both occur


def tokens(n, seed):
    return torch.randint(0, 512, (n,), generator=torch.Generator().manual_seed(seed))


def engine(batch=W * G, width=W, pages=N, stop=(), seed=SEED, length_penalty=1.0, **kw):
    """An empty batch (every row frozen until admitted) with beams of `width` (None: off)."""
    import _page_engine as E
    from qserve_amd.decode import TINY, DecodeEngine
    e = DecodeEngine(TINY, batch=batch, prompt_len=CAP_P, max_new=MAX_NEW, device="cuda:0", seed=seed, page_pool=pages, share_pages=True, **kw)
    e.enable_drafting(None, **E.NGRAM)
    e.set_stopping(stop, 0)
    if width is not None:
        e.set_beams(width, length_penalty)
    return e


def admit_groups(e, max_new=30, prompts=None):
    """Group 0 behind a prompt of P0 tokens, group 1 behind one of P1, in one admit each."""
    prompts = prompts or [tokens(P0, 1), tokens(P1, 2)]
    for g, X in enumerate(prompts):
        e.admit([g * W], [X], max_new_tokens=max_new, chunk=CHUNK, copy_rows=[list(range(g * W + 1, g * W + W))])
    return prompts


def state(e):
    """What two identical runs must agree on, bit for bit (the pool's snapshot without `tables`: they hold each engine's own addresses,
    and `page_ids` says the same)."""
    torch.cuda.synchronize()
    snap = {k: v for k, v in e.pager.snapshot().items() if k != "tables"}
    return dict(tokens=e.tokens.cpu(), beam_score=e.beam_score.cpu().view(torch.int32), history=e.history.cpu(), lengths=e.lengths.cpu(),
                finished=e.finished.cpu(), **{k: torch.as_tensor(v) for k, v in snap.items()})


def main():
    import _page_engine as E
    import _page_ref_cases as R
    eager, cap = engine(), engine()
    for e in (eager, cap):
        admit_groups(e)
    cap.capture()                                                           # (its warm-up is a real round)
    eager.step()
    for i in range(9):
        cap.run()
        eager.step()
        a, b = state(cap), state(eager)
        for k in a:
            assert torch.equal(a[k], b[k]), f"replay {i}: {k} differs"
    assert cap.lengths.tolist() == [P0 + 11] * W + [P1 + 11] * W and bool(torch.isfinite(cap.beam_score).all())
    assert len({tuple(r) for r in cap.history[:W, P0:P0 + 11].tolist()}) == W   # three hypotheses, not one text three times
    R.check_invariant(E.pool_state(cap))
    cap.check()
    print("BEAM-CAPTURE-OK")


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), here]
    main()
