"""The setting of tests/test_prefix_engine_gpu.py - TINY, B = 3, a counted pool of 12 pages under a prefix cache, and the pooled twin
without one - and, run as a program, the body of its capture test: the captured step of a prefix-cache engine replayed across a page
boundary.  That test starts this file in a fresh Python process for the reason tests/_page_engine.py gives: a failed capture leaves the
HIP context unusable.  The helpers of tests/_page_engine.py are used read-only.

X is a prompt of 150 tokens; Y = X[:128] + 61 tokens of its own (P = 189: lengths 190 behind the admit, so the fourth step writes slot
192, into a fourth page).  With X admitted first, Y maps X's two whole pages and runs ONE pass of 61 tokens at past 128 - the launch
that is the second pass of a twin that admits Y uncached in chunks of 128."""
import os
import sys

import torch

B, CAP_P, MAX_NEW, N, CHUNK = 3, 189, 40, 12, 128


def tokens(n, seed):
    return torch.randint(0, 512, (n,), generator=torch.Generator().manual_seed(seed))


X = tokens(150, 1)
Y = torch.cat((X[:128], tokens(61, 2)))


def engine(prefix_cache):
    import _page_engine as E
    from qserve_amd.decode import TINY, DecodeEngine
    e = DecodeEngine(TINY, batch=B, prompt_len=CAP_P, max_new=MAX_NEW, device="cuda:0", seed=5, page_pool=N, prefix_cache=prefix_cache)
    e.enable_drafting(None, **E.NGRAM)
    e.set_stopping((), 0)                                                   # every row frozen until it is admitted
    return e


def pair():
    """(the prefix-cache engine with X in row 0 and Y in row 1, the twin with Y in row 1)."""
    a, twin = engine(True), engine(False)
    a.admit([0], [X], max_new_tokens=MAX_NEW - 2, chunk=CHUNK)
    a.admit([1], [Y], max_new_tokens=MAX_NEW - 2, chunk=CHUNK)
    twin.admit([1], [Y], max_new_tokens=MAX_NEW - 2, chunk=CHUNK)
    return a, twin


def pool_state(eng):
    import _page_engine as E
    return E.pool_state(eng)


def page_bytes(eng, ids):
    """The bytes of the pages `ids` in every layer's K and V pool, on the host."""
    return [pool[ids].cpu() for pair_ in eng.pools for pool in pair_]


def main():
    import _page_engine as E
    import _page_ref_cases as R
    a, twin = pair()
    shared = a.pager.page_ids[1, :2].tolist()
    before = page_bytes(a, shared)
    for e in (a, twin):
        e.step()
        e.step()                                                            # lengths 192: the next two steps write slots 191 and 192
    a.capture()                                                             # (its warm-up is a real step)
    twin.step()
    E.assert_same_rows(a, twin, "after capture", rows=[1])
    for i in range(2):
        a.run()
        twin.step()
        E.assert_same_rows(a, twin, f"replay {i}", rows=[1])
    assert a.pager.owned.tolist() == [3, 4, 0] and a.pager.free_pages() == N - 5
    assert all(torch.equal(x, y) for x, y in zip(before, page_bytes(a, shared)))
    R.check_invariant(pool_state(a), cache=shared)
    a.check()
    print("PREFIX-CAPTURE-OK")


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), here]
    main()
