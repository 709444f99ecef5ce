"""The three rules of constrained decoding (include/qserve_amd.h: qs_constrain_node_states, qs_constrain_rows, qs_constrain_advance)
restated in numpy, a brute-force form of each in plain Python, and the case tables of tests/test_constrain_rows_cpu.py and
tests/test_constrain_rows_gpu.py.  Everything is integer: the device must agree bit for bit.

A case's tables: `token_class` int16 [n_vocab], `next` int32 [S, next_stride] of which the first C columns are the table (the rest
is padding that must never be read into a result: it holds non-negative values, so a leak allows what the table refuses)."""
import functools

import numpy as np

DEAD = -2
NEG_INF = 0xFC00
PAR = [-1, 0, 0, 0, 1, 1, 2, 4, 4, 5, 7, 7]              # the 12-node tree of tests/_accept_engine.py


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def move(st, t, token_class, nxt, C):
    """T(st, t) of the header comment."""
    S = nxt.shape[0]
    if not 0 <= st < S:
        return int(st)
    if not 0 <= t < len(token_class):
        return DEAD
    c = int(token_class[t])
    if not 0 <= c < C or nxt[st, c] < 0:
        return DEAD
    return int(nxt[st, c])


def restate_node_states(state, node_tokens, parents, token_class, nxt, C):
    B, n = node_tokens.shape
    out = np.empty((B, n), dtype=np.int32)
    for b in range(B):
        out[b, 0] = state[b]
        for i in range(1, n):
            a = parents[i] if 0 <= parents[i] < i else 0
            out[b, i] = move(int(out[b, a]), int(node_tokens[b, i]), token_class, nxt, C)
    return out


def restate_rows(store, n_vocab, row_state, token_class, nxt, C):
    """store uint16 [rows, stride] -> the masked copy: vectorised over the row."""
    out = store.copy()
    cls = token_class.astype(np.int64)
    in_range = (cls >= 0) & (cls < C)
    for r, s in enumerate(row_state):
        if 0 <= s < nxt.shape[0]:
            ok = in_range.copy()
            ok[in_range] = nxt[s, cls[in_range]] >= 0
            out[r, :n_vocab][~ok] = NEG_INF
    return out


def restate_advance(state, node_state, accept_idx, accept_lens, next_token, token_class, nxt, C, max_accept=1):
    out = state.copy()
    for b in range(len(state)):
        k = 1 if accept_lens is None else min(max(int(accept_lens[b]), 0), max_accept)
        if k == 0:
            continue
        if node_state is None or accept_idx is None:
            st = int(state[b])
        else:
            st = int(node_state[b, min(max(int(accept_idx[b, k - 1]), 0), node_state.shape[1] - 1)])
        if 0 <= st < nxt.shape[0]:
            out[b] = move(st, int(next_token[b]), token_class, nxt, C)
    return out


# ---- brute force: no shared code with the restatement beyond the table lookups ------------------------------------------------------
def brute_node_state(b, i, state, node_tokens, parents, token_class, nxt, C):
    """The state of node i by walking its path from the root, token by token."""
    path = []
    while i != 0:
        path.append(i)
        i = parents[i] if 0 <= parents[i] < i else 0
    st = int(state[b])
    for j in reversed(path):
        if st < 0 or st >= nxt.shape[0]:
            break
        t = int(node_tokens[b, j])
        allowed = 0 <= t < len(token_class) and 0 <= token_class[t] < C and nxt[st, token_class[t]] >= 0
        st = int(nxt[st, token_class[t]]) if allowed else DEAD
    return st


def brute_rows(store, n_vocab, row_state, token_class, nxt, C):
    out = store.copy()
    for r in range(store.shape[0]):
        s = int(row_state[r])
        if s < 0 or s >= nxt.shape[0]:
            continue
        for t in range(n_vocab):
            c = int(token_class[t])
            if c < 0 or c >= C or nxt[s, c] < 0:
                out[r, t] = NEG_INF
    return out


# ---- cases ------------------------------------------------------------------------------------------------------------------------------
def _logits(rng, rows, n_vocab, stride):
    """fp16 rows with positive, negative, +-0 and -inf values; the padding holds the canary 0x7BFF (65 504), the storage is exactly
    rows * stride elements."""
    x = (rng.standard_normal((rows, stride)) * 4).astype(np.float16)
    sel = rng.integers(0, 16, size=x.shape)
    x[sel == 0] = -np.inf
    x[sel == 1] = 0.0
    x[sel == 2] = -0.0
    bits = x.view(np.uint16).copy()
    bits[:, n_vocab:] = 0x7BFF
    return bits


def _automaton(rng, n_vocab, S, C, next_stride, allowed, odd_classes=()):
    """Random tables: a fraction `allowed` of the entries names a state; classes uniform in 0 .. C-1, `odd_classes` planted."""
    token_class = rng.integers(0, C, size=n_vocab).astype(np.int16)
    for j, c in enumerate(odd_classes):
        token_class[(7 * j + 3) % n_vocab::max(1, n_vocab // 5)] = c
    store = rng.integers(0, S, size=(S, next_stride)).astype(np.int32)        # (the padding: states, i.e. "allowed")
    store[:, :C][rng.random((S, C)) >= allowed] = -1
    store[:, :C][rng.random((S, C)) < 0.05] = -7                              # any negative entry refuses
    return token_class, store


CHUNK = 4096                                               # ids one pass of a constrain_rows workgroup covers (CR_CHUNK)
MIN_WORKGROUPS = 1024                                      # CR_MIN_WORKGROUPS


def launch_plan(n_vocab, C, rows):
    """The rule of qs_constrain_rows' launcher, restated: -> (ids per slice, slices per row).  A workgroup makes slice / CHUNK passes
    over its slice.  A change of the rule in csrc/constrain_rows.hip must be made here too: SLICES below pins what every row case
    is meant to launch, so that the cases go on covering one pass, several passes and a partial last slice."""
    chunks = -(-n_vocab // CHUNK)
    wanted = min(chunks, max(-(-n_vocab // (4 * C)), -(-MIN_WORKGROUPS // rows)))
    slice_ids = -(-chunks // wanted) * CHUNK
    return slice_ids, -(-n_vocab // slice_ids)


# case -> (ids per slice, slices per row) by launch_plan
SLICES = {"min_vocab": (4096, 1), "odd_tail": (4096, 1), "two_vectors_c3": (4096, 9), "two_vectors_c32768": (4096, 9),
          "big_vocab": (4096, 32), "passes_2": (8192, 5), "passes_5": (20480, 2)}


@functools.lru_cache(maxsize=None)
def row_cases():
    """name -> dict(store, n_vocab, row_state, token_class, next (the stored [S, next_stride]), C).  Built once per process: nobody
    writes into a case."""
    rng = np.random.default_rng(11)
    cases = {}
    # n_vocab = 8, S = 2, C = 1: state 0 allows everything, state 1 nothing; rows that are unconstrained, dead and out of range
    cases["min_vocab"] = dict(store=_logits(rng, 5, 8, 8), n_vocab=8, row_state=np.array([-1, DEAD, 2, 0, 1], dtype=np.int32),
                              token_class=np.zeros(8, dtype=np.int16), next=np.array([[1], [-1]], dtype=np.int32), C=1)
    # n_vocab % 8 != 0: the last ids are edited one by one, the padding behind them is not touched
    tc, nx = _automaton(rng, 12, 3, 4, 4, 0.5, odd_classes=(-1, 4))
    cases["odd_tail"] = dict(store=_logits(rng, 4, 12, 16), n_vocab=12, row_state=np.array([0, 1, 2, -1], dtype=np.int32),
                             token_class=tc, next=nx, C=4)
    # 33 000 ids at stride 33 008: nine slices of one chunk at C = 3 and, the rows being few, at C = 32 768 (the largest) too; classes
    # -1 and >= C; next_stride > C
    tc, nx = _automaton(rng, 33000, 4, 3, 5, 0.6, odd_classes=(-1, 3, 32767, -32768))
    cases["two_vectors_c3"] = dict(store=_logits(rng, 6, 33000, 33008), n_vocab=33000,
                                   row_state=np.array([0, 1, -1, 2, 3, 4], dtype=np.int32), token_class=tc, next=nx, C=3)
    tc, nx = _automaton(rng, 33000, 3, 32768, 32776, 0.5, odd_classes=(-1, -300))
    tc[:4] = (0, 32767, 31, 32)
    cases["two_vectors_c32768"] = dict(store=_logits(rng, 4, 33000, 33008), n_vocab=33000,
                                       row_state=np.array([2, DEAD, 0, 1], dtype=np.int32), token_class=tc, next=nx, C=32768)
    # the full vocabulary once: B = 2, n = 4 -> 8 rows
    tc, nx = _automaton(rng, 128256, 6, 256, 256, 0.3, odd_classes=(-1,))
    cases["big_vocab"] = dict(store=_logits(rng, 8, 128256, 128256), n_vocab=128256,
                              row_state=np.array([0, 1, 2, 3, 4, 5, -1, 6], dtype=np.int32), token_class=tc, next=nx, C=256)
    # SEVERAL PASSES per workgroup, what a verification at C > 1024 launches: 33 003 ids (n_vocab % 8 = 3) at stride 33 008.
    # passes_2: 128 rows at C = 32 768 -> slices of 8192 ids, two passes; the fifth and last slice holds 235 ids, 3 of them the tail.
    # passes_5: 512 rows at C = 8192 -> slices of 20 480 ids, five passes (the loop is unrolled by two: two pairs and one more); the
    # second and last slice holds 12 523 ids: three full passes, a partial one, the tail.  Its classes are CONTIGUOUS runs of ids
    # (neighbouring lanes read the same mask word), where every other case scatters them.  Every 8th row unconstrained, dead or out
    # of range
    tc, nx = _automaton(rng, 33003, 5, 32768, 32768, 0.5, odd_classes=(-1, -300))
    rs = rng.integers(0, 5, size=128).astype(np.int32)
    rs[3::8] = np.resize(np.array([-1, DEAD, 5], dtype=np.int32), rs[3::8].shape)
    cases["passes_2"] = dict(store=_logits(rng, 128, 33003, 33008), n_vocab=33003, row_state=rs, token_class=tc, next=nx, C=32768)
    _, nx = _automaton(rng, 33003, 5, 8192, 8200, 0.5)
    tc = (np.arange(33003, dtype=np.int64) * 8192 // 33003).astype(np.int16)
    tc[[0, 4095, 4096, 20479, 20480, 33000, 33002]] = (-1, 8192, 0, 8191, -1, 8191, 8192)     # (at the seams of passes and slices)
    rs = rng.integers(0, 5, size=512).astype(np.int32)
    rs[5::8] = np.resize(np.array([-1, DEAD, 5], dtype=np.int32), rs[5::8].shape)
    cases["passes_5"] = dict(store=_logits(rng, 512, 33003, 33008), n_vocab=33003, row_state=rs, token_class=tc, next=nx, C=8192)
    return cases


def small_automaton(rng, n_vocab=64, S=5, C=7, allowed=0.75):
    """class = token % C with a few tokens of class -1 and >= C; next_stride = C + 1."""
    token_class = (np.arange(n_vocab) % C).astype(np.int16)
    token_class[[5, 17]] = (-1, C)
    store = rng.integers(0, S, size=(S, C + 1)).astype(np.int32)
    store[:, :C][rng.random((S, C)) >= allowed] = -1
    return token_class, store, C


def node_cases():
    """name -> dict(state, node_tokens, parents, token_class, next, C)."""
    rng = np.random.default_rng(12)
    tc, nx, C = small_automaton(rng)
    V, S = len(tc), nx.shape[0]
    cases = {}
    # the 12-node tree: siblings with different tokens, special tokens, a disallowed node with children, an unconstrained root
    toks = rng.integers(0, V, size=(6, len(PAR))).astype(np.int64)
    toks[0, 2] = -1                                                           # node 2 dead -> its child 6 dead
    toks[0, 5] = V
    toks[1, 1] = 1 << 40                                                      # node 1 dead -> 4, 5, 7, 8, 9, 10, 11 dead
    toks[1, 3] = 5                                                            # class -1
    toks[3, 4] = 17                                                           # class >= C
    bad = next(c for c in range(C) if nx[2, c] < 0) if (nx[2, :C] < 0).any() else 0
    toks[4, 1] = bad                                                          # not allowed in the root's state 2
    live = [1] + [DEAD] * (len(PAR) - 1)                                      # sequence 5: every node holds a token its parent allows
    for i in range(1, len(PAR)):
        ok = [c for c in range(C) if live[PAR[i]] >= 0 and nx[live[PAR[i]], c] >= 0]
        if ok:
            toks[5, i] = ok[i % len(ok)] + C * (i % 4)                        # (siblings differ wherever two classes are allowed)
            toks[5, i] += C if toks[5, i] in (5, 17) else 0                   # (the two tokens whose class is not token % C)
            live[i] = int(nx[live[PAR[i]], ok[i % len(ok)]])
    cases["par12"] = dict(state=np.array([0, 3, -1, S, 2, 1], dtype=np.int32), node_tokens=toks, parents=PAR, token_class=tc, next=nx, C=C)
    # a 64-node chain: sequence 0 follows allowed tokens as long as there are any, sequence 1 is random, sequence 2 dead from the start
    chain = [-1] + list(range(63))
    toks = rng.integers(0, V, size=(3, 64)).astype(np.int64)
    st = 1
    for i in range(1, 64):
        ok = [c for c in range(C) if nx[st, c] >= 0]
        if not ok:
            break
        toks[0, i] = ok[i % len(ok)] + C * (i % 3)
        toks[0, i] += C if toks[0, i] in (5, 17) else 0
        st = int(nx[st, ok[i % len(ok)]])
    cases["chain64"] = dict(state=np.array([1, 4, DEAD], dtype=np.int32), node_tokens=toks, parents=chain, token_class=tc, next=nx, C=C)
    # parent entries outside 0 .. i-1: the node hangs off the root, its children go through it
    cases["malformed"] = dict(state=np.array([0, 2], dtype=np.int32), node_tokens=rng.integers(0, V, size=(2, 8)).astype(np.int64),
                              parents=[-1, 5, 1, -3, 3, 99, 6, 2], token_class=tc, next=nx, C=C)
    cases["root_only"] = dict(state=np.array([3, -1], dtype=np.int32), node_tokens=rng.integers(0, V, size=(2, 1)).astype(np.int64),
                              parents=[-1], token_class=tc, next=nx, C=C)
    return cases


def advance_cases():
    """name -> dict(state, node_state, accept_idx, accept_lens, next_token, max_accept, token_class, next, C)."""
    rng = np.random.default_rng(13)
    tc, nx, C = small_automaton(rng)
    V, S = len(tc), nx.shape[0]
    n = m = 6
    B = 10
    node_state = rng.integers(0, S, size=(B, n)).astype(np.int32)
    node_state[6, 2] = -1
    node_state[7, 1] = DEAD
    idx = rng.integers(0, n, size=(B, m)).astype(np.int32)
    idx[4, 2] = 100                                                           # clamped to n - 1
    idx[5, 0] = -5                                                            # clamped to 0
    idx[6, 1], idx[7, 0] = 2, 1
    lens = np.array([0, m, 3, 1, 3, 1, 2, 1, m + 5, -3], dtype=np.int32)      # frozen, full, clipped ..., beyond max_accept, negative
    tok = rng.integers(0, V, size=B).astype(np.int64)
    tok[2], tok[3], tok[8] = -1, V, 1 << 40                                   # out of the vocabulary: dead
    state = rng.integers(0, S, size=B).astype(np.int32)
    base = dict(token_class=tc, next=nx, C=C)
    cases = {"path": dict(state=state, node_state=node_state, accept_idx=idx, accept_lens=lens, next_token=tok, max_accept=m, **base),
             "path_no_lens": dict(state=state, node_state=node_state, accept_idx=idx, accept_lens=None, next_token=tok, max_accept=m, **base)}
    state = np.array([0, 1, 2, 3, 4, -1, DEAD, S, 0, 1], dtype=np.int32)
    cases["step"] = dict(state=state, node_state=None, accept_idx=None, accept_lens=None, next_token=tok, max_accept=1, **base)
    cases["step_k"] = dict(state=state, node_state=None, accept_idx=None, accept_lens=np.array([1, 0] * 5, dtype=np.int32), next_token=tok,
                           max_accept=1, **base)
    return cases


# ---- byte-level DFAs built by hand (tests/test_constrain_rows_cpu.py) ------------------------------------------------------------------
def byte_dfa(edges, n_states, accepting):
    """edges: (state, bytes of the allowed byte values, next state) -> (trans int32 [n_states, 256], accepting bool [n_states])."""
    trans = np.full((n_states, 256), -1, dtype=np.int32)
    for s, chars, d in edges:
        for ch in chars:
            trans[s, ch] = d
    acc = np.zeros(n_states, dtype=bool)
    acc[list(accepting)] = True
    return trans, acc


DIGITS = b"0123456789"


def dfa_digits():
    """digits+"""
    return byte_dfa([(0, DIGITS, 1), (1, DIGITS, 1)], 2, [1])


def dfa_int_list():
    r"""\[\d+(,\d+)*\]"""
    return byte_dfa([(0, b"[", 1), (1, DIGITS, 2), (2, DIGITS, 2), (2, b",", 1), (2, b"]", 3)], 4, [3])


def dfa_choice(words=(b"yes", b"yeah")):
    """A choice list as a trie."""
    edges, nodes, acc = [], {b"": 0}, []
    for w in words:
        for i in range(1, len(w) + 1):
            if w[:i] not in nodes:
                nodes[w[:i]] = len(nodes)
            edges.append((nodes[w[:i - 1]], w[i - 1:i], nodes[w[:i]]))
        acc.append(nodes[w])
    return byte_dfa(edges, len(nodes), acc)


def synthetic_vocab(rng, size=512):
    """`size` byte strings of 1 .. 4 bytes over the alphabet the hand-made DFAs speak (and a few bytes they do not), with duplicates and
    an empty string; the last id is the eos token (its bytes never matter)."""
    alphabet = np.frombuffer(b"0123456789[],yesah x", dtype=np.uint8)
    vocab = [bytes(rng.choice(alphabet, size=int(rng.integers(1, 5))).tolist()) for _ in range(size)]
    for t, w in enumerate((b"[", b"]", b",", b"7", b"42", b"yes", b"ye", b"ah", b"s", b"y", b"yeah", b"1,2", b"[1", b"9]")):
        vocab[t] = w
    vocab[20], vocab[21], vocab[22] = b"", vocab[3], vocab[4]                  # an empty string; duplicates
    vocab[size - 1] = b"</s>"
    return vocab, size - 1


def brute_token_matrix(trans, accepting, vocab, eos_id, n_vocab):
    """[Sb + 1, n_vocab] by running every token's bytes in plain Python."""
    Sb = trans.shape[0]
    m = np.full((Sb + 1, n_vocab), -1, dtype=np.int64)
    for s in range(Sb):
        for t, w in enumerate(vocab):
            if t == eos_id or len(w) == 0:
                continue
            cur = s
            for ch in w:
                cur = int(trans[cur, ch])
                if cur < 0:
                    break
            m[s, t] = cur
        if accepting[s]:
            m[s, eos_id] = Sb
    m[Sb, eos_id] = Sb
    return m


def dfa_matrix(dfa):
    """The [S, V] token transition matrix a TokenDFA stands for (-1 wherever it refuses, whatever negative value it stores)."""
    cls, nxt = dfa.token_class.numpy().astype(np.int64), dfa.next.numpy().astype(np.int64)
    m = np.full((nxt.shape[0], len(cls)), -1, dtype=np.int64)
    ok = (cls >= 0) & (cls < nxt.shape[1])
    m[:, ok] = np.maximum(nxt[:, cls[ok]], -1)
    return m
