"""Pooled engines, their static twins and the state comparison shared by tests/test_page_pool_engine_gpu.py - and, run as a program,
the body of its capture test: two replays of the captured step of a pooled engine against the eager steps of a static twin.  The
capture test starts this file in a fresh Python process because a failed capture leaves the HIP context unusable.

Setting: TINY, B = 3, P = 125, seed 5 - a prefill leaves lengths of 126, so the third step and a 12-node tree behind the second cross
slot 128 into a third page.  A pooled engine and its twin differ in where their pages lie, never in what they hold: the comparison reads
every row's slots through the pooled engine's `page_ids` and through the twin's own tables."""
import os
import sys

import torch

B, P, MAX_NEW = 3, 125, 40
PAR = [-1, 0, 0, 0, 1, 1, 2, 4, 4, 5, 7, 7]
NGRAM = dict(max_ngram=3, min_match=1, pad_token=7)


def prompt(gpu):
    from qserve_amd.decode import TINY
    return torch.randint(0, TINY["vocab"], (B * P,), device=gpu, generator=torch.Generator(device=gpu).manual_seed(1))


def engine(page_pool=None):
    from qserve_amd.decode import TINY, DecodeEngine
    return DecodeEngine(TINY, batch=B, prompt_len=P, max_new=MAX_NEW, device="cuda:0", seed=5, page_pool=page_pool)


def page_ids(eng, li, kv):
    """int64 [B, mb] on the host: the page index behind every table entry of layer li (a pooled engine: its sink where none is owned)."""
    return ((eng.tables[li][:, kv] - eng.pools[li][kv].data_ptr()) // eng.page_bytes).cpu()


def row_slots(eng, b, upto, layers=None):
    """The bytes of slots 0 .. upto - 1 of row b, every layer (or those of `layers`), K and V: per page the data rows [Hkv, slots, bytes], then the fp16 scales
    and zeros [Hkv, slots] of those slots (the page layout of oracle/kvattn.py) -> a list of uint8 tensors on the host."""
    hkv, dhb = eng.Hkv, eng.size_per_token // eng.Hkv
    data_end = hkv * 64 * dhb
    out = []
    for li in (range(len(eng.layers)) if layers is None else layers):
        for kv in range(2):
            ids = page_ids(eng, li, kv)[b].tolist()
            if eng.pager is not None:                                        # the tables say what page_ids says
                own = eng.pager.page_ids[b].cpu().tolist()
                assert ids == [i if i >= 0 else eng.pager.N for i in own], f"row {b}, layer {li}: tables and page_ids disagree"
            pool = eng.pools[li][kv]
            for j in range((upto + 63) // 64):
                cnt = min(64, upto - 64 * j)
                assert eng.pager is None or ids[j] < eng.pager.N, f"row {b}: slot {64 * j} lies in the sink"
                page = pool[ids[j]].cpu()
                out.append(page[:data_end].view(hkv, 64, dhb)[:, :cnt].contiguous())
                out.append(page[data_end:].view(2, hkv, 64, 2)[:, :, :cnt].contiguous())
    return out


def assert_same_rows(a, b, what, rows=range(B), hidden=True):
    """tokens, lengths, hidden and the slots < lengths - 1 of `rows`, byte for byte."""
    torch.cuda.synchronize()
    lens = a.lengths.cpu().tolist()
    for r in rows:
        assert int(a.tokens[r]) == int(b.tokens[r]), f"{what}: row {r} tokens differ"
        assert lens[r] == int(b.lengths[r]), f"{what}: row {r} lengths differ"
        assert not hidden or torch.equal(a.hidden[r].view(torch.int16), b.hidden[r].view(torch.int16)), f"{what}: row {r} hidden differs"
        for i, (x, y) in enumerate(zip(row_slots(a, r, lens[r] - 1), row_slots(b, r, lens[r] - 1))):
            assert torch.equal(x, y), f"{what}: row {r} slots differ (piece {i})"


def pool_state(eng):
    """The pool's snapshot in the form tests/_page_cases.check_invariant takes."""
    p = eng.pager
    return dict(p.snapshot(), bases=p.layer_bases.cpu().numpy(), N=p.N, mb=p.mb, page_bytes=p.page_bytes)


def main():
    """prefill and two steps (lengths 128), capture() - whose warm-up is a real step -, two replays: the second and third page
    boundary crossing happen under the graph.  The twin steps eagerly."""
    gpu = torch.device("cuda:0")
    toks = prompt(gpu)
    cap, twin = engine(page_pool=12), engine()
    for e in (cap, twin):
        e.prefill(P, toks)
        e.step()
        e.step()
    cap.capture()
    twin.step()
    assert_same_rows(cap, twin, "after capture")
    for i in range(2):
        cap.run()
        twin.step()
        assert_same_rows(cap, twin, f"replay {i}")
    assert cap.pager.owned.tolist() == [3, 3, 3] and cap.pager.free_pages() == 3
    cap.check()
    print("CAPTURE-OK")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    main()
