"""Engines with stopping on, the cut of an unstopped twin's text by the numpy rule, and the bytes of a sequence's page slots, shared by
tests/test_stopping_gpu.py - and, run as a program, the bodies of its capture and generate tests (`capture` / `generate` as the
argument).  Those start this file in a fresh Python process because a failed capture leaves the HIP context unusable and
nothing else may share it.

Setting of tests/_speculate_engine.py: TINY, B = 3, P = 70, max_new = 40, seed 5, the 12-node tree PAR, n-gram drafting."""
import os
import sys

import torch

import _accept_engine as E
import _speculate_engine as S
from _stop_cases import NO_LIMIT, assemble, restate_loop, row, table

CAP = E.P + 40                                           # the history's capacity: prompt_len + max_new
SAMPLING = ((0.8, 50, 0.9), dict(seed=3))                # set_sampling of the capture program


def stopping_engine(toks, stop, max_new_tokens=None):
    e = S.drafting_engine(toks)
    e.set_stopping(stop, max_new_tokens)
    return e


def texts_of(e):
    """The text of every sequence as a list (prompt included)."""
    torch.cuda.synchronize()
    h, lens = e.history.cpu(), e.lengths.cpu().tolist()
    return [h[b, :n].tolist() for b, n in enumerate(lens)]


def cut(text, stops, max_new):
    """Where the numpy rule ends the text `text` (prompt of P tokens, then what an engine without stopping generated): the rule is
    applied the way set_stopping and step() apply it - once to the first generated token with check_root, then to one new token at a
    time.  -> (length, reason); reason 0: the text ran out before anything stopped."""
    T = table([[s] if isinstance(s, int) else list(s) for s in stops]) if stops else None
    limit = NO_LIMIT if max_new is None else E.P + max_new
    first = assemble([row("first", text[:E.P + 1], plen=E.P, limit=limit, m=0)], T, n=1, cap=CAP, check_root=1)
    reason = int(restate_loop(first)["finished"][0])
    L = E.P + 1
    while reason == 0 and L < len(text):
        out = restate_loop(assemble([row("step", text[:L], bonus=text[L], plen=E.P, limit=limit)], T, n=1, cap=CAP, step=True))
        L += int(out["accept_lens"][0])
        reason = int(out["finished"][0])
    return L, reason


def assert_cut_of(e, twin_texts, stops, max_new, what):
    """Every sequence of `e` holds the twin's text cut by the rule (or all of it so far, if nothing has stopped it yet), ends in its
    current token, and `finished` says why.  -> the expected (length, reason) pairs."""
    got, fin, toks = texts_of(e), e.finished.cpu().tolist(), e.tokens.cpu().tolist()
    want = []
    for b, text in enumerate(twin_texts):
        L, reason = cut(text, stops, None if max_new is None else max_new[b])
        want.append((L, reason))
        if reason == 0:                                                      # still live: e may not be behind the twin
            assert len(got[b]) == len(text), f"{what}: sequence {b} holds {len(got[b])} tokens, the unstopped twin {len(text)}"
        assert got[b] == text[:L], f"{what}: sequence {b}: {got[b][E.P:]} is not the twin's {text[E.P:]} cut at {L - E.P}"
        assert fin[b] == reason, f"{what}: sequence {b}: finished = {fin[b]}, expected {reason}"
        assert toks[b] == got[b][-1], f"{what}: sequence {b} does not end in its current token"
    return want


def slot_bytes(e, b, upto):
    """The bytes of slots 0 .. upto - 1 of sequence b in every layer's K and V pages - data, scale, zero - as one uint8 tensor."""
    dhb, Hkv, mb = (64 if e.int4 else 128), e.Hkv, e.mb
    out = []
    for (kp, vp), t in zip(e.pools, e.tables):
        for which, pool in enumerate((kp, vp)):
            blocks = ((t[b, which] - pool.data_ptr()) // e.page_bytes).to(torch.int64)
            pages = pool[blocks]                                             # [mb, page_bytes]
            data = pages[:, :Hkv * 64 * dhb].reshape(mb, Hkv, 64, dhb).permute(0, 2, 1, 3).reshape(mb * 64, -1)
            par = pages[:, Hkv * 64 * dhb:].reshape(mb, 2, Hkv, 64, 2).permute(0, 3, 1, 2, 4).reshape(mb * 64, -1)
            out += [data[:upto].reshape(-1), par[:upto].reshape(-1)]
    return torch.cat(out).cpu()


class Frozen:
    """Watches an engine round by round: from the round after a sequence finished, its `tokens`, `lengths`, text and page slots
    < lengths stay byte-equal to the end; slots < lengths - 1 from the finishing round itself (the last token's K / V is written by
    the round that follows)."""

    def __init__(self, e):
        self.e, self.kept = e, {}

    def look(self, what):
        e = self.e
        torch.cuda.synchronize()
        fin, lens, toks = e.finished.cpu().tolist(), e.lengths.cpu().tolist(), e.tokens.cpu().tolist()
        for b, f in enumerate(fin):
            if f == 0:
                assert b not in self.kept, f"{what}: sequence {b} is live again"
                continue
            L = lens[b]
            state = (f, L, toks[b], e.history[b, :L].cpu())
            if b not in self.kept:
                self.kept[b] = dict(state=state, rounds=0, below=slot_bytes(e, b, L - 1))
                continue
            k = self.kept[b]
            k["rounds"] += 1
            assert state[:3] == k["state"][:3] and torch.equal(state[3], k["state"][3]), f"{what}: the frozen sequence {b} changed"
            assert torch.equal(slot_bytes(e, b, L - 1), k["below"]), f"{what}: page slots < lengths - 1 of the frozen sequence {b} changed"
            if k["rounds"] == 1:
                k["all"] = slot_bytes(e, b, L)
            else:
                assert torch.equal(slot_bytes(e, b, L), k["all"]), f"{what}: page slots < lengths of the frozen sequence {b} changed"

    def checked(self):
        """Sequences whose slots < lengths were compared across at least two frozen rounds."""
        return sorted(b for b, k in self.kept.items() if k["rounds"] >= 2)


def assert_same(a, b, what):
    """State, text and finish reasons of two stopping engines."""
    E.assert_same_state(a, b, what)
    S.assert_same_text(a, b, what)
    assert torch.equal(a.finished, b.finished), f"{what}: finished differs"


def capture_main():
    """capture() and capture_speculate() with stopping on against an eager twin, the sampling head on (the greedy text of the tiny model
    soon repeats one token, which leaves nothing to tell stop tables apart by): the stop id is what an unstopped scout emits two steps
    on, sequence 1 has five tokens to go.  Then a new table through set_stopping under the captured graph: the next replay follows it,
    an engine that kept the old table does not."""
    gpu = torch.device("cuda:0")
    toks = E.prompt(gpu)
    scout = S.drafting_engine(toks)
    scout.set_sampling(*SAMPLING[0], **SAMPLING[1])
    for _ in range(2):
        scout.step()
    stop = [int(scout.tokens[0])]
    new = [40, 5, 40]
    cap, twin, ref, old = (stopping_engine(toks, stop, new) for _ in range(4))
    for e in (cap, twin, ref, old):
        e.set_sampling(*SAMPLING[0], **SAMPLING[1])
    cap.capture()                                            # (its warm-up is a real step)
    for e in (twin, ref, old):
        e.step()
    assert_same(cap, twin, "after capture")
    for i in range(2):
        cap.run()
        for e in (twin, ref, old):
            e.step()
        assert_same(cap, twin, f"captured step {i}")
    assert int(cap.finished[0]) == 1 and int(cap.lengths[0]) <= E.P + 3, "the scout's token did not stop sequence 0 where the scout emitted it"
    cap.capture_speculate(E.PAR, sampled=True)
    for e in (twin, ref, old):
        e.speculate(E.PAR, sampled=True)
    assert_same(cap, twin, "after capture_speculate")
    S.plant(ref, (cap, twin, old))
    for i in range(2):
        got = cap.run_speculate()
        want = twin.speculate(E.PAR, sampled=True)
        old.speculate(E.PAR, sampled=True)
        torch.cuda.synchronize()
        E.assert_same_result(got, want, f"replay {i}")
        assert_same(cap, twin, f"replay {i}")
        print(f"replay {i}: accepted path lengths {got[1].tolist()}, finished {cap.finished.tolist()}")
        assert int(got[1][0]) == 0, "the frozen sequence 0 accepted something"
        if i == 0:
            assert int(got[1].max()) >= 2, "the planted continuation was accepted nowhere: the replay checked root-only paths"
    # (sequence 1 ends at its limit at the latest - the stop id may come first: the rule decides, and the twin agreed above)
    assert int(cap.finished[1]) != 0 and int(cap.lengths[1]) <= E.P + 5 and int(cap.finished[2]) == 0
    # a new table under the captured graph.  The engine with the old table runs three rounds ahead and tells what sequence 2 is about to
    # emit: the first token that differs from its current one becomes the table (so that set_stopping's own look at the current token
    # finds nothing), and the replays must end the sequence exactly there
    L2 = int(twin.lengths[2])
    first = None                                             # sequence 2's length after the first of these rounds
    for _ in range(3):
        old.speculate(E.PAR, sampled=True)
        first = int(old.lengths[2]) if first is None else first
    ahead = texts_of(old)[2]
    assert int(old.finished[2]) == 0
    j = next((j for j in range(L2, len(ahead)) if ahead[j] != ahead[L2 - 1]), None)
    assert j is not None, f"the setting gives no token to stop at: sequence 2 repeats {ahead[L2 - 1]}"
    for e in (cap, twin):
        e.set_stopping([[ahead[j]]], new)
    assert int(cap.finished[2]) == 0
    for i in range(3):
        got = cap.run_speculate()
        want = twin.speculate(E.PAR, sampled=True)
        torch.cuda.synchronize()
        E.assert_same_result(got, want, f"replay {i} with the new table")
        assert_same(cap, twin, f"replay {i} with the new table")
        if i == 0:                                           # the next replay: it ends the sequence if it emits the token, else all goes on
            assert (int(cap.finished[2]), int(cap.lengths[2])) == ((1, j + 1) if j < first else (0, first)), \
                "the table that was filled under the captured graph did not take effect on the next replay"
    assert int(cap.finished[2]) == 1 and texts_of(cap)[2] == ahead[:j + 1] and int(cap.tokens[2]) == ahead[j], \
        "the table that was filled under the captured graph did not end sequence 2 where the rule ends it"
    print("STOP-CAPTURE-OK")


def generate_main():
    """generate() over the captured step graph and over the captured speculate graph against unstopped twins, and with page tables that
    (by the bound) have no room for another round."""
    gpu = torch.device("cuda:0")
    toks = E.prompt(gpu)
    # -- steps: 12 of an unstopped twin give the texts; sequence 0 stops at what it emits at step 3, the others by length
    twin = S.drafting_engine(toks)
    for _ in range(12):
        twin.step()
    full = texts_of(twin)
    stop, new = [full[0][E.P + 3]], [10, 6, 8]
    e = stopping_engine(toks, stop, new)
    e.capture()                                              # (a real step; generate counts the rounds it replays itself)
    texts, reasons, rounds, reads = e.generate(40, poll_every=4)
    want = assert_cut_of(e, full, stop, new, "generate over steps")
    assert all(r != 0 for r in reasons) and reasons == [r for _, r in want] and reasons == e.finished.tolist()
    assert rounds < 40 and rounds % 4 == 0 and reads == -(-rounds // 4), f"{rounds} rounds, {reads} read-backs"
    assert texts == [full[b][E.P:L] for b, (L, _) in enumerate(want)]
    assert e._len_bound == max(L for L, _ in want)
    print(f"steps: {rounds} rounds, {reads} read-backs, reasons {reasons}, generated {[len(t) for t in texts]}")
    # -- speculation: the twin speculates eagerly, unstopped; generate captures the round itself
    twin = S.drafting_engine(toks)
    for _ in range(14):
        twin.speculate(E.PAR)
        twin.sync_length_bound()                             # (the bound grows by the whole tree per round otherwise)
    full = texts_of(twin)
    stop, new = [full[0][E.P + 4], full[1][E.P + 6:E.P + 8]], [40, 40, 9]
    e = stopping_engine(toks, stop, new)
    texts, reasons, rounds, reads = e.generate(40, parents=E.PAR, poll_every=3)
    want = assert_cut_of(e, full, stop, new, "generate over speculation")
    assert all(r != 0 for r in reasons) and reasons == [r for _, r in want]
    assert rounds < 40 and reads == -(-rounds // 3), f"{rounds} rounds, {reads} read-backs"
    assert texts == [full[b][E.P:L] for b, (L, _) in enumerate(want)]
    print(f"speculation: {rounds} rounds, {reads} read-backs, reasons {reasons}, generated {[len(t) for t in texts]}")
    # -- no room: by the bound another tree does not fit the page tables - generate returns, it does not assert
    e.set_stopping([], None)                                 # (everything live again)
    assert e.finished.tolist() == [0, 0, 0]
    e._len_bound = e.mb * 64 - 3
    before = texts_of(e)
    texts, reasons, rounds, reads = e.generate(40, parents=E.PAR, poll_every=3)
    assert (rounds, reads, reasons) == (0, 0, [0, 0, 0]) and texts_of(e) == before and texts == [t[E.P:] for t in before]
    e._len_bound = e.mb * 64 - 2 * len(E.PAR)                # room for two rounds: the burst of three is shortened to them, the
    texts, reasons, rounds, reads = e.generate(3, parents=E.PAR, poll_every=3)      # read-back makes room for the third
    assert (rounds, reads) == (3, 2) and e._len_bound == int(e.lengths.max())
    # -- a step graph captured before stopping was switched on holds no stop launch: generate captures again
    e = S.drafting_engine(toks)
    e.capture()
    without = e.graph
    e.set_stopping([], 4)
    _, reasons, rounds, reads = e.generate(8, poll_every=4)
    assert e.graph is not without and reasons == [2, 2, 2] and e.lengths.tolist() == [E.P + 4] * 3 and (rounds, reads) == (4, 1)
    print("STOP-GENERATE-OK")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    {"capture": capture_main, "generate": generate_main}[sys.argv[1]]()
