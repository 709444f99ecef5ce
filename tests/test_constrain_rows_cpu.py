"""Constrained decoding on the CPU: the numpy restatement of the three rules (tests/_constraint_cases.py, what the GPU tests compare
bits with) against a brute-force walk in plain Python, and the host-side compiler `constraints.TokenDFA.from_byte_dfa` / `union` on
byte DFAs built by hand, checked against running every token's bytes one by one."""
import numpy as np
import pytest

import _constraint_cases as K


@pytest.fixture(scope="module")
def constraints(built_lib):
    from qserve_amd import constraints
    return constraints


# ---- the restatement against brute force -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["par12", "chain64", "malformed", "root_only"])
def test_node_states_restatement_against_a_walk_of_every_path(name):
    c = K.node_cases()[name]
    C, nxt = c["C"], c["next"]
    got = K.restate_node_states(c["state"], c["node_tokens"], c["parents"], c["token_class"], nxt, C)
    B, n = c["node_tokens"].shape
    for b in range(B):
        for i in range(n):
            assert got[b, i] == K.brute_node_state(b, i, c["state"], c["node_tokens"], c["parents"], c["token_class"], nxt, C), (b, i)
    assert np.array_equal(got[:, 0], c["state"])


def test_node_cases_plant_what_they_say():
    cases = K.node_cases()
    c = cases["par12"]
    st = K.restate_node_states(c["state"], c["node_tokens"], c["parents"], c["token_class"], c["next"], c["C"])
    assert st[0, 2] == K.DEAD and st[0, 6] == K.DEAD                       # a dead node's child is dead
    assert all(st[1, i] == K.DEAD for i in (1, 4, 5, 7, 8, 9, 10, 11)) and st[1, 3] == K.DEAD
    assert (st[2] == -1).all() and (st[3] == c["next"].shape[0]).all()     # unconstrained roots: the whole tree keeps the root's value
    assert st[4, 1] == K.DEAD
    alive = st[(st >= 0) & (st < c["next"].shape[0])]
    assert alive.size >= 12, "hardly any node of the case is alive"
    ch = cases["chain64"]
    st = K.restate_node_states(ch["state"], ch["node_tokens"], ch["parents"], ch["token_class"], ch["next"], ch["C"])
    assert st[0, 63] >= 0 and (st[2] == K.DEAD).all()                      # the planted chain lives to its end


@pytest.mark.parametrize("name", ["min_vocab", "odd_tail"])
def test_rows_restatement_against_a_loop_over_every_logit(name):
    c = K.row_cases()[name]
    got = K.restate_rows(c["store"], c["n_vocab"], c["row_state"], c["token_class"], c["next"], c["C"])
    assert np.array_equal(got, K.brute_rows(c["store"], c["n_vocab"], c["row_state"], c["token_class"], c["next"], c["C"]))
    assert np.array_equal(got[:, c["n_vocab"]:], c["store"][:, c["n_vocab"]:])
    for r, s in enumerate(c["row_state"]):
        if not 0 <= s < c["next"].shape[0]:
            assert np.array_equal(got[r], c["store"][r])


@pytest.mark.parametrize("name", ["passes_2", "passes_5"])
def test_rows_restatement_on_the_long_cases_row_by_row(name):
    """The loop over every logit on a handful of rows of the cases too large for it: constrained ones and one that is not."""
    c = K.row_cases()[name]
    S = c["next"].shape[0]
    off = next(r for r, s in enumerate(c["row_state"]) if not 0 <= s < S)
    pick = [0, 1, off, len(c["row_state"]) - 1]
    got = K.restate_rows(c["store"][pick], c["n_vocab"], c["row_state"][pick], c["token_class"], c["next"], c["C"])
    assert np.array_equal(got, K.brute_rows(c["store"][pick], c["n_vocab"], c["row_state"][pick], c["token_class"], c["next"], c["C"]))
    assert np.array_equal(got[2], c["store"][off]) and (got[0] != c["store"][0]).any()


def test_every_row_case_launches_what_it_says():
    """The launcher's slicing rule (restated in _constraint_cases.launch_plan, its two constants read from the kernel file) on every row
    case: one pass per workgroup in the small cases, two and five passes with a partial last slice and an n_vocab % 8 tail in the two
    that exist for it - so a change of the rule that takes the several-pass path out of the tests shows here."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "qserve_amd", "csrc", "constrain_rows.hip")).read()
    threads = int(re.search(r"constexpr int CR_THREADS = (\d+);", src).group(1))
    assert re.search(r"constexpr int CR_CHUNK = CR_THREADS \* 8;", src) and threads * 8 == K.CHUNK
    assert int(re.search(r"constexpr int CR_MIN_WORKGROUPS = (\d+);", src).group(1)) == K.MIN_WORKGROUPS
    cases = K.row_cases()
    assert set(cases) == set(K.SLICES)
    for name, c in cases.items():
        assert K.launch_plan(c["n_vocab"], c["C"], len(c["row_state"])) == K.SLICES[name], name
    for name, passes in (("passes_2", 2), ("passes_5", 5)):
        c, (ids, slices) = cases[name], K.SLICES[name]
        last = c["n_vocab"] - (slices - 1) * ids
        assert ids == passes * K.CHUNK and slices >= 2 and 0 < last < ids and c["n_vocab"] % 8 != 0 and c["store"].shape[1] > c["n_vocab"]
        assert c["C"] > 1024 and ((c["row_state"] >= 0) & (c["row_state"] < c["next"].shape[0])).sum() > len(c["row_state"]) // 2
    # what the engine launches in a verification of 64 sequences x 12 nodes at the largest C: 16 passes
    assert K.launch_plan(128256, 32768, 768) == (16 * K.CHUNK, 2) and K.launch_plan(128256, 256, 768) == (K.CHUNK, 32)


def test_min_vocab_has_an_all_allowed_and_a_none_allowed_state():
    c = K.row_cases()["min_vocab"]
    got = K.restate_rows(c["store"], 8, c["row_state"], c["token_class"], c["next"], 1)
    assert np.array_equal(got[:3], c["store"][:3]) and np.array_equal(got[3], c["store"][3]) and (got[4] == K.NEG_INF).all()


@pytest.mark.parametrize("name", ["path", "path_no_lens", "step", "step_k"])
def test_advance_restatement_by_hand(name):
    c = K.advance_cases()[name]
    got = K.restate_advance(c["state"], c["node_state"], c["accept_idx"], c["accept_lens"], c["next_token"], c["token_class"], c["next"],
                            c["C"], c["max_accept"])
    S, m = c["next"].shape[0], c["max_accept"]
    for b in range(len(got)):
        k = 1 if c["accept_lens"] is None else int(np.clip(c["accept_lens"][b], 0, m))
        if k == 0:
            assert got[b] == c["state"][b]
            continue
        st = c["state"][b] if c["node_state"] is None else c["node_state"][b, int(np.clip(c["accept_idx"][b, k - 1], 0, c["node_state"].shape[1] - 1))]
        if not 0 <= st < S:
            assert got[b] == c["state"][b]
            continue
        t = int(c["next_token"][b])
        cls = c["token_class"][t] if 0 <= t < len(c["token_class"]) else -1
        want = c["next"][st, cls] if 0 <= cls < c["C"] and c["next"][st, cls] >= 0 else K.DEAD
        assert got[b] == want, b
    if name == "path":
        assert got[2] == K.DEAD and got[3] == K.DEAD and got[0] == c["state"][0] and got[6] == c["state"][6] and got[7] == c["state"][7]


# ---- from_byte_dfa -------------------------------------------------------------------------------------------------------------------
DFAS = {"digits": K.dfa_digits, "int_list": K.dfa_int_list, "choice": K.dfa_choice}


@pytest.mark.parametrize("name", sorted(DFAS))
@pytest.mark.parametrize("chunk_states", [1, 64])
def test_from_byte_dfa_against_running_every_tokens_bytes(constraints, name, chunk_states):
    trans, acc = DFAS[name]()
    vocab, eos = K.synthetic_vocab(np.random.default_rng(21))
    n_vocab = len(vocab) + 8                                                # ids beyond the vocabulary: never allowed
    dfa = constraints.TokenDFA.from_byte_dfa(trans, acc, vocab, eos, n_vocab=n_vocab, chunk_states=chunk_states)
    want = K.brute_token_matrix(trans, acc, vocab, eos, n_vocab)
    assert dfa.S == trans.shape[0] + 1 and dfa.V == n_vocab
    assert str(dfa.token_class.dtype) == "torch.int16" and str(dfa.next.dtype) == "torch.int32"
    assert np.array_equal(K.dfa_matrix(dfa), want)
    # the classes are the distinct columns; a token no state allows has class -1
    cols = {tuple(col) for col in want.T.tolist() if max(col) >= 0}
    assert dfa.C == len(cols)
    cls = dfa.token_class.numpy()
    assert ((cls < 0) == (want.max(axis=0) < 0)).all() and cls.max() == dfa.C - 1
    assert cls[20] == -1 and (cls[len(vocab):] == -1).all()               # the empty string; ids beyond the vocabulary
    assert cls[21] == cls[3] and cls[22] == cls[4]                        # duplicates share a class
    assert (want >= 0).sum() > dfa.S, "the vocabulary hardly speaks the DFA's language"


def test_every_negative_transition_is_no_transition(constraints):
    """`trans` entries below -1 refuse like -1 and make no classes of their own: the same DFA with its missing transitions spelt -1,
    -2, -7 ... at random gives the very same tables."""
    trans, acc = K.dfa_int_list()
    vocab, eos = K.synthetic_vocab(np.random.default_rng(21))
    want = constraints.TokenDFA.from_byte_dfa(trans, acc, vocab, eos)
    noisy = np.where(trans < 0, -np.random.default_rng(22).integers(1, 9, size=trans.shape), trans).astype(np.int32)
    assert (noisy < -1).sum() > 100
    got = constraints.TokenDFA.from_byte_dfa(noisy, acc, vocab, eos)
    assert got.C == want.C and np.array_equal(got.token_class.numpy(), want.token_class.numpy())
    assert np.array_equal(got.next.numpy(), want.next.numpy()) and got.next.min() == -1


def test_eos_and_the_sink(constraints):
    trans, acc = K.dfa_int_list()
    vocab, eos = K.synthetic_vocab(np.random.default_rng(21))
    dfa = constraints.TokenDFA.from_byte_dfa(trans, acc, vocab, eos)
    m, sink = K.dfa_matrix(dfa), trans.shape[0]
    for s in range(trans.shape[0]):
        assert m[s, eos] == (sink if acc[s] else -1)
    assert m[sink, eos] == sink and (np.delete(m[sink], eos) == -1).all()
    assert (m[:sink] != sink)[:, np.arange(len(vocab)) != eos].all()       # nothing but eos reaches the sink
    assert dfa.allowed(sink).sum() == 1 and dfa.allowed(-1).all() and dfa.allowed(3)[eos]
    # walking "[42,7]" token by token ends in the accepting state, and then only eos goes on
    st = 0
    for w in (b"[", b"42", b",", b"7", b"]"):
        assert dfa.allowed(st)[vocab.index(w)]
        st = int(m[st, vocab.index(w)])
    assert acc[st] and dfa.allowed(st)[eos]
    # without an accepting state eos is allowed by the sink alone and still has a class of its own
    none = constraints.TokenDFA.from_byte_dfa(trans, np.zeros_like(acc), vocab, eos)
    mm = K.dfa_matrix(none)
    assert (mm[:sink, eos] == -1).all() and mm[sink, eos] == sink


def test_union_keeps_every_part_at_its_offset(constraints):
    vocab, eos = K.synthetic_vocab(np.random.default_rng(21))
    parts = [constraints.TokenDFA.from_byte_dfa(*f(), vocab, eos) for f in (K.dfa_digits, K.dfa_int_list, K.dfa_choice)]
    both, offsets = constraints.TokenDFA.union(parts)
    assert offsets == [0, parts[0].S, parts[0].S + parts[1].S] and both.S == sum(p.S for p in parts)
    m = K.dfa_matrix(both)
    for p, off in zip(parts, offsets):
        want = K.dfa_matrix(p)
        assert np.array_equal(m[off:off + p.S], np.where(want >= 0, want + off, -1))
    stack = np.stack([p.token_class.numpy() for p in parts])
    assert both.C == len({tuple(c) for c in stack.T.tolist() if max(c) >= 0})
    with pytest.raises(ValueError):
        constraints.TokenDFA.union([parts[0], constraints.TokenDFA.from_byte_dfa(*K.dfa_digits(), vocab[:100], 99)])


def test_more_than_32768_classes_are_refused(constraints):
    """Two-byte tokens (hi, lo) over a 26-state DFA whose start state i asks for bit i of the token: states 0 .. 7 test a bit of hi and
    take any lo, states 8 .. 15 take any hi and test a bit of lo.  Token t's column over those 16 states spells t in binary, so every
    token has a column of its own: 65 535 classes are refused, 32 767 tokens and eos are exactly the 32 768 that fit."""
    A, B0, F = 16, 17, 25
    trans = np.full((26, 256), -1, dtype=np.int32)
    byte = np.arange(256)
    for i in range(8):
        trans[i, byte[(byte >> i) & 1 == 1]] = A                            # bit i of hi, then any lo
        trans[8 + i, :] = B0 + i                                            # any hi, then bit i of lo
        trans[B0 + i, byte[(byte >> i) & 1 == 1]] = F
    trans[A, :] = F
    acc = np.zeros(26, dtype=bool)
    acc[F] = True
    vocab = [bytes((t >> 8, t & 255)) for t in range(65536)] + [b"<eos>"]
    with pytest.raises(ValueError, match="32768"):
        constraints.TokenDFA.from_byte_dfa(trans, acc, vocab, eos_id=65536)
    dfa = constraints.TokenDFA.from_byte_dfa(trans, acc, vocab[:32768] + [b"<eos>"], eos_id=32768)
    assert dfa.C == 32768 and dfa.token_class[0] == -1 and len(set(dfa.token_class.tolist())) == 32769
    m = K.dfa_matrix(dfa)
    assert m[3, 8 << 8] == F and m[3, 7 << 8] == -1 and m[9, 2] == F and m[9, 1] == -1 and m[F, 32768] == 26
