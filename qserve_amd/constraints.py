"""Constrained decoding (extension; NOT part of the reference's `qserve_backend` surface): a token automaton restricts what every
sequence may emit, on the device and capturable in a hipGraph - nothing crosses to the host between tokens, and the rows of a draft
tree are masked each with the state of its own node.

    TokenDFA        the two tables on the host - token_class int16 [V], next int32 [S, C] - built from a byte-level DFA and a vocabulary
                    (`from_byte_dfa`), several grammars joined into one table (`union`), `.to(device)`.
    node_states     the automaton state of every node of a draft tree: the state reached along the path root -> node.
    constrain_rows  fp16 logit rows in place: -inf wherever the row's state does not allow the token; in front of `argmax_rows_` /
                    `sampling.sample_rows`, behind `penalties.penalize_rows`.
    advance         the per-sequence state after a round, from the walk's outputs (the arrays of `drafting.history_append`).

include/qserve_amd.h (`qs_constrain_node_states`, `qs_constrain_rows`, `qs_constrain_advance`) has the rules; a numpy restatement is
bit-equal (tests/_constraint_cases.py).  Backed by qserve_amd/csrc/constrain_rows.hip.  DecodeEngine.set_constraint puts them into the
engine's rounds."""
import numpy as np
import torch

from .backend._util import check, expect, guard, lib, ptr, stream
from .drafting import MAX_TREE, _rows, _typed

DEAD = -2                      # QS_FSM_DEAD: what a transition over a token that is not allowed yields (unconstrained, like -1)
MAX_CLASSES = 32768


def _tables(token_class, nxt, what):
    """The checks every entry makes of the tables -> (V, S, C, next_stride, device)."""
    _typed(token_class, torch.int16, "token_class")
    _typed(nxt, torch.int32, "next")
    if token_class.dim() != 1 or token_class.numel() < 8:
        raise RuntimeError(f"{what}: token_class must be [n_vocab] with n_vocab >= 8, got {tuple(token_class.shape)}")
    if nxt.dim() != 2 or nxt.size(0) < 1 or not 1 <= nxt.size(1) <= MAX_CLASSES or (nxt.size(1) > 1 and nxt.stride(1) != 1) or \
            (nxt.size(0) > 1 and nxt.stride(0) < nxt.size(1)):
        raise RuntimeError(f"{what}: next must be [S, C] (S >= 1, 1 <= C <= {MAX_CLASSES}) with a unit column stride and a row stride "
                           f">= C, got {tuple(nxt.shape)}, strides {nxt.stride()}")
    dev = token_class.device
    if nxt.device != dev:
        raise RuntimeError(f"{what}: next must be on {dev}, got {nxt.device}")
    expect(token_class, torch.int16, "token_class")
    expect(nxt, torch.int32, "next", contiguous=False)
    return token_class.numel(), nxt.size(0), nxt.size(1), max(nxt.stride(0), nxt.size(1)), dev


def node_states(state, node_tokens, parents, token_class, next, out=None):
    """out[b, i] = the automaton state of node i of sequence b (int32 [B, n]): out[b, 0] = state[b] (int32 [B]), and for i >= 1 the
    state of its parent moved over node_tokens[b, i] (int64 [B, n]; column 0 is not read) in the tree parents int32 [n] (parents[0] = -1;
    n <= 64; an entry not in 0 .. i-1 hangs the node off the root).  A state outside 0 .. S-1 is unconstrained and stays what it is;
    a token that is out of the vocabulary or not allowed yields DEAD (-2).  Tables: token_class int16 [V], next int32 [S, C] (rows may
    be padded).  -> out."""
    what = "constraints.node_states"
    V, S, C, nstride, dev = _tables(token_class, next, what)
    _typed(state, torch.int32, "state")
    if state.dim() != 1 or state.device != dev:
        raise RuntimeError(f"{what}: state must be [B] on {dev}, got {tuple(state.shape)} on {state.device}")
    B = state.numel()
    _typed(node_tokens, torch.int64, "node_tokens")
    if node_tokens.dim() != 2 or node_tokens.size(0) != B or not 1 <= node_tokens.size(1) <= MAX_TREE or node_tokens.device != dev:
        raise RuntimeError(f"{what}: node_tokens must be [{B}, 1 .. {MAX_TREE}] on {dev}, got {tuple(node_tokens.shape)} on "
                           f"{node_tokens.device}")
    n = node_tokens.size(1)
    _rows(parents, torch.int32, (n,), "parents", dev, what)
    if out is None:
        out = torch.empty((B, n), dtype=torch.int32, device=dev)
    _typed(out, torch.int32, "out")
    if out.numel() != B * n or out.device != dev:
        raise RuntimeError(f"{what}: out must hold [{B}, {n}] on {dev}, got {tuple(out.shape)} on {out.device}")
    for t, name in ((state, "state"), (node_tokens, "node_tokens"), (parents, "parents"), (out, "out")):
        expect(t, t.dtype, name)
    if B == 0:
        return out
    with guard(state):
        check(lib.qs_constrain_node_states(ptr(state), ptr(node_tokens), ptr(parents), ptr(token_class), V, ptr(next), nstride, S, C, B, n,
                                           ptr(out), stream()), what)
    return out


def constrain_rows(logits, row_state, token_class, next):
    """Mask the fp16 rows logits [rows, V] in place: for every row r whose row_state[r] (int32 [rows]) is a state s in 0 .. S-1, every
    logit of a token t with a class outside 0 .. C-1 or with next[s, token_class[t]] < 0 becomes -inf; every other element keeps its
    bits.  Rows of a state outside 0 .. S-1 (-1: unconstrained, -2: DEAD) and the padding behind V are not written.  Rows need V >= 8,
    a unit column stride, a row stride that is a multiple of 8 and a 16-byte aligned start; V = token_class.numel().  -> logits."""
    what = "constraints.constrain_rows"
    V, S, C, nstride, dev = _tables(token_class, next, what)
    _typed(logits, torch.float16, "logits")
    if logits.dim() != 2 or (logits.size(1) > 1 and logits.stride(1) != 1):
        raise RuntimeError(f"{what}: logits must be [rows, n] with a unit column stride, got {tuple(logits.shape)}, strides {logits.stride()}")
    rows, n = logits.shape
    row_stride = max(logits.stride(0), n) if rows <= 1 else logits.stride(0)
    if n != V:
        raise RuntimeError(f"{what}: logits have {n} columns, token_class names {V} tokens")
    if row_stride < n or row_stride % 8 != 0:
        raise RuntimeError(f"{what}: the row stride {row_stride} must be a multiple of 8 that is >= n={n}")
    if logits.device != dev:
        raise RuntimeError(f"{what}: logits must be on {dev}, got {logits.device}")
    _rows(row_state, torch.int32, (rows,), "row_state", dev, what)
    expect(logits, torch.float16, "logits", contiguous=False)
    expect(row_state, torch.int32, "row_state")
    if rows == 0:
        return logits
    with guard(logits):
        check(lib.qs_constrain_rows(ptr(logits), row_stride, n, ptr(row_state), ptr(token_class), ptr(next), nstride, S, C, rows, stream()),
              what)
    return logits


def advance(state, next_token, token_class, next, node_state=None, accept_idx=None, accept_lens=None):
    """state[b] (int32 [B], in place) after a round that emitted k = accept_lens[b] tokens (int32 [B]; None: 1), the last of them
    next_token[b] (int64 [B]): the state of the row that emitted it - node_state[b, accept_idx[b, k - 1]] (int32 [B, n] / int32
    [B, max_accept], what `node_states` and the walk left; both None: state[b], a plain step) - moved over next_token[b].  k == 0 and a
    state outside 0 .. S-1 write nothing; a token that is out of the vocabulary or not allowed yields DEAD.  Runs behind the walk and
    behind `stopping.stop_update`, whose clipped k and next_token it then sees.  -> state."""
    what = "constraints.advance"
    V, S, C, nstride, dev = _tables(token_class, next, what)
    _typed(state, torch.int32, "state")
    if state.dim() != 1 or state.device != dev:
        raise RuntimeError(f"{what}: state must be [B] on {dev}, got {tuple(state.shape)} on {state.device}")
    B = state.numel()
    _rows(next_token, torch.int64, (B,), "next_token", dev, what)
    if (node_state is None) != (accept_idx is None):
        raise RuntimeError(f"{what}: node_state and accept_idx come together (a verification) or not at all (a step)")
    n = max_accept = 1
    if node_state is not None:
        for t, name in ((node_state, "node_state"), (accept_idx, "accept_idx")):
            _typed(t, torch.int32, name)
            if t.dim() != 2 or t.size(0) != B or not 1 <= t.size(1) <= MAX_TREE or t.device != dev:
                raise RuntimeError(f"{what}: {name} must be [{B}, 1 .. {MAX_TREE}] on {dev}, got {tuple(t.shape)} on {t.device}")
        n, max_accept = node_state.size(1), accept_idx.size(1)
    if accept_lens is not None:
        _rows(accept_lens, torch.int32, (B,), "accept_lens", dev, what)
    for t, name in ((state, "state"), (next_token, "next_token"), (node_state, "node_state"), (accept_idx, "accept_idx"),
                    (accept_lens, "accept_lens")):
        if t is not None:
            expect(t, t.dtype, name)
    if B == 0:
        return state
    with guard(state):
        check(lib.qs_constrain_advance(ptr(state), ptr(node_state), ptr(accept_idx), ptr(accept_lens), ptr(next_token), ptr(token_class), V,
                                       ptr(next), nstride, S, C, B, n, max_accept, stream()), what)
    return state


def _first_seen(labels):
    """Renumber integer labels 0, 1, ... in the order of their first occurrence (negative labels stay)."""
    labels = np.asarray(labels)
    out = labels.copy()
    live = labels >= 0
    if live.any():
        uniq, first, inv = np.unique(labels[live], return_index=True, return_inverse=True)
        rank = np.empty(len(uniq), dtype=np.int64)
        rank[np.argsort(first, kind="stable")] = np.arange(len(uniq))
        out[live] = rank[inv.reshape(-1)]
    return out


class TokenDFA:
    """A token automaton on the host: `token_class` int16 [V] (the class of every token id, -1: never allowed) and `next` int32 [S, C]
    (the state after a token of class c in state s, negative: not allowed).  `S`, `C`, `V` are its sizes.  `.to(device)` -> a TokenDFA
    whose two tensors live there (what the entries of this module and DecodeEngine.set_constraint take)."""

    def __init__(self, token_class, next):
        token_class, next = torch.as_tensor(token_class), torch.as_tensor(next)
        if token_class.dtype != torch.int16 or token_class.dim() != 1:
            raise ValueError(f"TokenDFA: token_class must be int16 [V], got {token_class.dtype} {tuple(token_class.shape)}")
        if next.dtype != torch.int32 or next.dim() != 2 or next.size(0) < 1 or not 1 <= next.size(1) <= MAX_CLASSES:
            raise ValueError(f"TokenDFA: next must be int32 [S, C] with S >= 1 and 1 <= C <= {MAX_CLASSES}, got {next.dtype} "
                             f"{tuple(next.shape)}")
        self.token_class, self.next = token_class.contiguous(), next.contiguous()

    V = property(lambda self: self.token_class.numel())
    S = property(lambda self: self.next.size(0))
    C = property(lambda self: self.next.size(1))

    def to(self, device):
        return TokenDFA(self.token_class.to(device), self.next.to(device))

    def allowed(self, s):
        """bool [V] on the host: which tokens state s allows (every one if s is outside 0 .. S-1)."""
        cls, nxt = self.token_class.cpu().numpy().astype(np.int64), self.next.cpu().numpy()
        if not 0 <= s < self.S:
            return np.ones(self.V, dtype=bool)
        ok = (cls >= 0) & (cls < self.C)
        ok[ok] = nxt[s, cls[ok]] >= 0
        return ok

    @staticmethod
    def _token_moves(trans, states, tok_bytes, tok_lens):
        """-> int32 [len(states), len(tok_lens)]: where every byte state of `states` lands after the bytes of every token (tok_bytes uint8
        [T, maxlen], tok_lens [T]; -1: some byte has no transition).  Vectorised over (state, token) per byte position."""
        cur = np.repeat(np.asarray(states, dtype=np.int32)[:, None], len(tok_lens), axis=1)
        for p in range(tok_bytes.shape[1]):
            cols = np.nonzero(tok_lens > p)[0]
            if cols.size == 0:
                break
            c = cur[:, cols]
            live = c >= 0
            step = trans[np.where(live, c, 0), tok_bytes[cols, p][None, :]]
            cur[:, cols] = np.where(live, step, -1)
        return cur

    @classmethod
    def from_byte_dfa(cls, trans, accepting, vocab, eos_id, n_vocab=None, chunk_states=64):
        """The token automaton of a byte-level DFA over a vocabulary.  `trans` int32 [Sb, 256]: the byte state after byte x in byte
        state s, -1 (or any negative value) for no transition; `accepting` bool [Sb]; `vocab`: a list of `bytes`, one per token id; `n_vocab`: the size of the
        model's vocabulary (default len(vocab); ids >= len(vocab) are never allowed).  Token state s is byte state s: a token moves s to
        the byte state reached by running all its bytes and is not allowed in s if any byte has no transition; a token with empty
        bytes is never allowed.  One extra sink state Sb: every accepting state allows `eos_id` (whatever its bytes), which moves to
        the sink, and the sink allows only `eos_id`, staying there.  Classes are the distinct columns of the [S, V] token transition
        matrix; tokens no state allows get class -1.  More than 32 768 classes: ValueError.  The matrix is built `chunk_states` states at
        a time, so a real vocabulary never needs S * V words at once."""
        trans = np.maximum(np.asarray(trans, dtype=np.int32), -1)     # (any negative entry is "no transition": ONE value, so
        #                                                               that columns differing only in it share a class)
        accepting = np.asarray(accepting, dtype=bool)
        if trans.ndim != 2 or trans.shape[1] != 256 or trans.shape[0] < 1 or accepting.shape != (trans.shape[0],):
            raise ValueError(f"from_byte_dfa: trans must be [Sb, 256] and accepting [Sb], got {trans.shape} and {accepting.shape}")
        Sb = trans.shape[0]
        if trans.max() >= Sb:
            raise ValueError(f"from_byte_dfa: trans names a byte state >= Sb = {Sb}")
        V = len(vocab) if n_vocab is None else int(n_vocab)
        if V < len(vocab) or not 0 <= int(eos_id) < V:
            raise ValueError(f"from_byte_dfa: n_vocab={V} must cover the {len(vocab)} tokens of vocab and eos_id={eos_id}")
        eos_id, sink = int(eos_id), Sb
        lens = np.zeros(V, dtype=np.int64)
        lens[:len(vocab)] = [len(w) for w in vocab]
        lens[eos_id] = 0                                   # (its column comes from the eos rule, not from its bytes)
        tok_bytes = np.zeros((V, max(1, int(lens.max()))), dtype=np.uint8)
        for t, w in enumerate(vocab):
            if lens[t]:
                tok_bytes[t, :lens[t]] = np.frombuffer(w, dtype=np.uint8)
        worded = np.nonzero(lens > 0)[0]                   # the tokens whose bytes are run

        def rows(states, tokens):
            """The token transition matrix of byte states `states` over `tokens` (ids), the eos column by its rule."""
            m = np.full((len(states), len(tokens)), -1, dtype=np.int32)
            w = np.nonzero(lens[tokens] > 0)[0]
            if w.size:
                m[:, w] = cls._token_moves(trans, states, tok_bytes[tokens[w]], lens[tokens[w]])
            e = np.nonzero(tokens == eos_id)[0]
            if e.size:
                m[:, e] = np.where(accepting[np.asarray(states)], sink, -1)[:, None].astype(np.int32)
            return m

        # pass 1: the classes, refined chunk by chunk - two tokens share a class iff their columns agree in every state
        live = np.union1d(worded, [eos_id])
        label = np.zeros(len(live), dtype=np.int64)
        ever = np.zeros(len(live), dtype=bool)             # allowed in some state
        for s0 in range(0, Sb, chunk_states):
            m = rows(np.arange(s0, min(Sb, s0 + chunk_states)), live)
            ever |= (m >= 0).any(axis=0)
            _, label = np.unique(np.vstack([label[None, :], m]), axis=1, return_inverse=True)
            label = label.reshape(-1)
        ever[live == eos_id] = True                        # the sink allows eos (alone: no other column holds the sink)
        label = _first_seen(np.where(ever, label, -1))
        C = int(label.max()) + 1 if (label >= 0).any() else 0
        if C > MAX_CLASSES:
            raise ValueError(f"from_byte_dfa: {C} token classes, the tables hold at most {MAX_CLASSES}")
        token_class = np.full(V, -1, dtype=np.int16)
        token_class[live] = label.astype(np.int16)
        # pass 2: one representative token per class gives the class's column
        C = max(C, 1)
        nxt = np.full((Sb + 1, C), -1, dtype=np.int32)
        reps = np.full(C, -1, dtype=np.int64)
        for t, c in zip(live[::-1], label[::-1]):
            if c >= 0:
                reps[c] = t
        have = np.nonzero(reps >= 0)[0]
        for s0 in range(0, Sb, chunk_states):
            nxt[s0:min(Sb, s0 + chunk_states), have] = rows(np.arange(s0, min(Sb, s0 + chunk_states)), reps[have])
        if token_class[eos_id] >= 0:
            nxt[sink, token_class[eos_id]] = sink
        return cls(torch.from_numpy(token_class), torch.from_numpy(nxt))

    @classmethod
    def union(cls, dfas):
        """Several automata over the same vocabulary as ONE table: part j's states are offsets[j] .. offsets[j] + S_j - 1, the classes
        the common refinement of the parts' classes (two tokens share a class iff they do in every part).  -> (TokenDFA, offsets)."""
        dfas = list(dfas)
        if not dfas or any(d.V != dfas[0].V for d in dfas):
            raise ValueError("TokenDFA.union: at least one automaton, all over the same vocabulary")
        parts = []
        for d in dfas:
            c = d.token_class.cpu().numpy().astype(np.int64)
            parts.append(np.where((c >= 0) & (c < d.C), c, -1))
        stack = np.stack(parts)                                              # [k, V]
        _, label = np.unique(stack, axis=1, return_inverse=True)
        label = np.where((stack >= 0).any(axis=0), label.reshape(-1), -1)
        label = _first_seen(label)
        C = int(label.max()) + 1 if (label >= 0).any() else 0
        if C > MAX_CLASSES:
            raise ValueError(f"TokenDFA.union: {C} token classes, the tables hold at most {MAX_CLASSES}")
        C = max(C, 1)
        reps = np.full(C, -1, dtype=np.int64)
        for t in range(len(label) - 1, -1, -1):
            if label[t] >= 0:
                reps[label[t]] = t
        have = np.nonzero(reps >= 0)[0]
        offsets, blocks, off = [], [], 0
        for d, c in zip(dfas, parts):
            src = d.next.cpu().numpy()
            blk = np.full((d.S, C), -1, dtype=np.int32)
            pc = c[reps[have]]                                               # the part's class of every new class (-1: not allowed here)
            col = src[:, np.where(pc >= 0, pc, 0)]
            blk[:, have] = np.where((pc >= 0)[None, :] & (col >= 0), col + off, -1)
            offsets.append(off)
            blocks.append(blk)
            off += d.S
        return cls(torch.from_numpy(label.astype(np.int16)), torch.from_numpy(np.vstack(blocks))), offsets
