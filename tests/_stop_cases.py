"""The stop rule of `qs_stop_update` (include/qserve_amd.h) restated twice in numpy - a straight loop over text positions and an
independent array formulation -, a random case generator, and the named cases of tests/test_stop_update_gpu.py.

A CASE is one launch: a dict of numpy arrays under the argument names of qserve_amd.stopping.stop_update (None where the argument is
absent) plus `cap`, `n`, `max_accept`, `check_root` and `names` (one label per row).  The restatements return the four outputs:
accept_lens (k), next_token, last_row, finished."""
import numpy as np

NO_LIMIT = 2 ** 31 - 1
SENTINEL = -777                                           # last_row before the launch: "not written" is visible


def _clamp(v, lo, hi):
    return lo if v < lo else hi if v > hi else v


def _seq(case, b):
    """(L, m, plen) of row b, clamped as the header says."""
    cap = case["cap"]
    L = _clamp(int(case["lengths"][b]), 0, cap)
    mcap = min(case["max_accept"], 64)
    if case["node_tokens"] is None or case["accept_idx"] is None:
        mcap = 1
    m = 1 if case["accept_lens"] is None else _clamp(int(case["accept_lens"][b]), 0, mcap)
    plen = 0 if case["prompt_lens"] is None else max(int(case["prompt_lens"][b]), 0)
    return L, m, plen


def _outputs(case):
    B = len(case["lengths"])
    return dict(accept_lens=np.zeros((B,), np.int32), next_token=case["next_token"].copy(), last_row=case["last_row"].copy(),
                finished=case["finished"].copy())


def _table(case):
    if case["stop_seqs"] is None:
        return np.zeros((0, 1), np.int32), np.zeros((0,), np.int32)
    return case["stop_seqs"], case["stop_lens"]


def restate_loop(case):
    """The rule as the header words it: for every emitted index j, every table row, token by token."""
    out = _outputs(case)
    cap, n = case["cap"], case["n"]
    seqs, lens = _table(case)
    W = seqs.shape[1]
    for b in range(len(case["lengths"])):
        L, m, plen = _seq(case, b)

        def node(j):
            return _clamp(int(case["accept_idx"][b, j]), 0, n - 1)

        def e(j):
            return int(case["next_token"][b]) if j == m else int(case["node_tokens"][b, node(j)])

        def tok(p):
            if p < plen or p >= cap:
                return None
            return int(case["history"][b, p]) if p < L else e(p - L + 1)

        k, reason = m, 0
        if case["finished"][b] != 0:
            k = 0
        else:
            for j in range(m + 1):
                stop = False
                if j >= (0 if case["check_root"] else 1):
                    for s in range(seqs.shape[0]):
                        ln = int(lens[s])
                        if not 1 <= ln <= W or any(int(t) < 0 for t in seqs[s, :ln]):
                            continue
                        if all(tok(L - 1 + j - (ln - 1) + t) == int(seqs[s, t]) for t in range(ln)):
                            stop = True
                limited = case["limit_lens"] is not None and L + j >= int(case["limit_lens"][b])
                if stop or limited:
                    k, reason = j, 1 if stop else 2
                    break
            if reason:
                out["finished"][b] = reason
        out["accept_lens"][b] = k
        if k != m:
            if k >= 1:
                out["next_token"][b] = e(k)
                out["last_row"][b] = b * n + node(k - 1)
            elif L >= 1:
                out["next_token"][b] = int(case["history"][b, L - 1])
    return out


def restate_arrays(case):
    """Independently: the whole text of a sequence as one array, every table row slid over it, the hits as a vector over j."""
    out = _outputs(case)
    cap, n = case["cap"], case["n"]
    seqs, lens = _table(case)
    for b in range(len(case["lengths"])):
        L, m, plen = _seq(case, b)
        if m >= 1:
            nodes = np.clip(case["accept_idx"][b, 1:m], 0, n - 1) if m > 1 else np.zeros((0,), np.int64)
            emitted = np.concatenate([case["node_tokens"][b, nodes] if m > 1 else np.zeros((0,), np.int64), case["next_token"][b:b + 1]])
        else:
            nodes, emitted = np.zeros((0,), np.int64), np.zeros((0,), np.int64)
        text = np.concatenate([case["history"][b, :L].astype(np.int64), emitted.astype(np.int64)])
        pos = np.arange(L + m)
        real = (pos >= plen) & (pos < cap)
        ends = np.zeros((L + m + 1,), bool)                              # ends[q + 1]: a stop sequence ends at position q (ends[0]: q = -1)
        for s in range(seqs.shape[0]):
            ln = int(lens[s])
            if not 1 <= ln <= seqs.shape[1] or (seqs[s, :ln] < 0).any() or ln > L + m:
                continue
            w = np.lib.stride_tricks.sliding_window_view(text, ln)
            r = np.lib.stride_tricks.sliding_window_view(real, ln)
            ends[ln:] |= (w == seqs[s, :ln].astype(np.int64)).all(axis=1) & r.all(axis=1)
        j = np.arange(m + 1)
        stop = ends[L + j] & (j >= (0 if case["check_root"] else 1))
        limited = (L + j >= int(case["limit_lens"][b])) if case["limit_lens"] is not None else np.zeros((m + 1,), bool)
        hit = stop | limited
        if case["finished"][b] != 0:
            k = 0
        elif hit.any():
            k = int(np.argmax(hit))
            out["finished"][b] = 1 if stop[k] else 2
        else:
            k = m
        out["accept_lens"][b] = k
        if k < m and k >= 1:
            out["next_token"][b] = emitted[k - 1]
            out["last_row"][b] = b * n + int(np.clip(case["accept_idx"][b, k - 1], 0, n - 1))
        elif k < m and L >= 1:
            out["next_token"][b] = case["history"][b, L - 1]
    return out


# ---- building cases -------------------------------------------------------------------------------------------------------------------
def table(rows, S=None, W=None, pad=-1):
    """A stop table from lists of ids: S rows (default len(rows)) of W columns (default the longest); unused rows have length 0."""
    S = len(rows) if S is None else S
    W = max([len(r) for r in rows] + [1]) if W is None else W
    seqs, lens = np.full((S, W), pad, np.int32), np.zeros((S,), np.int32)
    for i, r in enumerate(rows):
        seqs[i, :len(r)] = r
        lens[i] = len(r)
    return seqs, lens


def row(name, text, path=(), bonus=0, plen=0, limit=NO_LIMIT, fin=0, length=None, m=None, idx=None):
    """One sequence: `text` = history[:L]; `path` = the tokens e_1 .. e_(m-1) of the accepted nodes, `bonus` = e_m.  `length`: lengths[b]
    where it is not len(text); `m`: accept_lens[b] where it is not len(path) + 1; `idx`: the accept_idx entries 1 .. where they are
    not the consecutive nodes 1, 2, ..."""
    return dict(name=name, text=list(text), path=list(path), bonus=bonus, plen=plen, limit=limit, fin=fin, length=length, m=m, idx=idx)


def assemble(rows, stops, n, cap, check_root=0, max_accept=None, step=False, limits=True, prompts=True, stride=None, fill=1000):
    """Rows -> one launch.  Node i of a sequence holds path[i - 1] (the accepted path is nodes 0, 1, 2, ... unless the row says
    otherwise); the other nodes and the history behind the text hold `fill` + something, which no stop table names.  `step`: the plain
    step of the engine - no draft, no path, accept_lens absent (m = 1)."""
    B = len(rows)
    max_accept = n if max_accept is None else max_accept
    stride = cap if stride is None else stride
    hist = (fill + np.arange(B * stride, dtype=np.int32).reshape(B, stride) % 50).astype(np.int32)
    lengths, plens, lims, fin = (np.zeros((B,), np.int32) for _ in range(4))
    nxt = np.zeros((B,), np.int64)
    nodes = (fill + 100 + np.arange(B * n, dtype=np.int64).reshape(B, n) % 37)
    idx = np.zeros((B, max_accept), np.int32)
    lens = np.zeros((B,), np.int32)
    for b, r in enumerate(rows):
        L = min(len(r["text"]), cap)
        hist[b, :L] = r["text"][:L]
        lengths[b] = len(r["text"]) if r["length"] is None else r["length"]
        plens[b], lims[b], fin[b], nxt[b] = r["plen"], r["limit"], r["fin"], r["bonus"]
        for i, t in enumerate(r["path"]):
            nodes[b, 1 + i] = t
        path_idx = list(range(1, len(r["path"]) + 1)) if r["idx"] is None else list(r["idx"])
        idx[b, 1:1 + len(path_idx)] = path_idx[:max_accept - 1]
        lens[b] = len(r["path"]) + 1 if r["m"] is None else r["m"]
    seqs, slens = stops if stops is not None else (None, None)
    return dict(names=[r["name"] for r in rows], cap=cap, n=n, max_accept=1 if step else max_accept, check_root=check_root,
                history=hist, lengths=lengths, prompt_lens=plens if prompts else None, node_tokens=None if step else nodes,
                accept_idx=None if step else idx, accept_lens=None if step else lens, next_token=nxt,
                last_row=np.full((B,), SENTINEL, np.int64), stop_seqs=seqs, stop_lens=slens, limit_lens=lims if limits else None,
                finished=fin)


def named_cases():
    """The launches of the GPU test, every row labelled.  Tokens 1 .. 99 are text, the stop tables name some of them."""
    T = table([[7], [3, 4], [9, 9, 9]])
    base = [11, 12, 13, 14, 15, 16]                                         # six tokens of text, the first four the prompt
    g = {}
    g["tree12"] = assemble([
        row("seam: [3, 4] ends at e_1, the 3 is the current token", base + [3], [4, 20, 21], 22, plen=4),
        row("a match that would begin inside the prompt", base + [3], [4, 20, 21], 22, plen=7),
        row("stop at e_1", base, [7, 20, 21, 22], 23, plen=4),
        row("stop at e_m, the bonus token", base, [20, 21, 22], 7, plen=4),
        row("none", base, [20, 21, 22], 23, plen=4),
        row("limit and stop on the same index", base, [20, 7, 21], 22, plen=4, limit=8),
        row("limit before stop", base, [20, 21, 7], 22, plen=4, limit=7),
        row("L >= limit on entry", base, [20, 21], 22, plen=4, limit=5),
    ], T, n=12, cap=48)
    g["tree12_state"] = assemble([
        row("already finished by a stop", base, [7, 20], 21, plen=4, fin=1),
        row("already finished by the length", base, [20, 21], 22, plen=4, fin=2, limit=100),
        row("accept_idx entries out of range", base, [20, 21, 22], 23, plen=4, idx=[-5, 99, 2]),
        row("out-of-range entry clamps onto the node that holds a stop", base, [20, 21], 22, plen=4, idx=[1, 99]),
        row("three-token stop over two history tokens and e_1", base + [9, 9], [9, 20], 21, plen=4),
        row("clip inside the path: last_row and next_token move", base, [20, 21, 7, 22, 23], 24, plen=4),
        row("accept_lens beyond max_accept", base, [20] * 11, 21, plen=4, m=99),
        row("negative accept_lens", base, [7], 7, plen=4, m=-2),
    ], T, n=12, cap=48, stride=56)
    g["tree12_state"]["node_tokens"][3, 11] = 7                              # what the clamped 99 lands on
    g["lengths"] = assemble([
        row("lengths beyond the cap", [30 + i for i in range(16)], [7, 20], 21, length=40),
        row("lengths beyond the cap, at the limit", [30 + i for i in range(16)], [20], 21, length=40, limit=17),
        row("negative lengths: no text, no frozen token to take", [], [20, 7], 21, length=-3, limit=0),
        row("negative lengths: the text is the emitted tokens alone", [], [20, 7], 21, length=-3),
        row("text fills the history: e_1 lies beyond the cap", [30 + i for i in range(16)], [7], 7),
        row("one slot left: e_1 is the last position that counts", [30 + i for i in range(15)], [7, 20], 7),
        row("one slot left: e_2 lies beyond the cap", [30 + i for i in range(15)], [20, 7], 7),
    ], T, n=12, cap=16, stride=16)
    g["root"] = assemble([
        row("check_root hit", base + [7], plen=4, m=0),
        row("check_root: the current token is still prompt", base + [7], plen=7, m=0),
        row("check_root: a two-token stop ending at the current token", base + [3, 4], plen=4, m=0),
        row("check_root: at the limit", base, plen=4, limit=6, m=0),
        row("check_root: live", base, plen=4, limit=7, m=0),
        row("check_root with a path: the root wins", base + [7], [7], 7, plen=4),
    ], T, n=12, cap=48, check_root=1)
    g["step"] = assemble([
        row("step: stop at the new token", base, bonus=7, plen=4),
        row("step: none", base, bonus=8, plen=4),
        row("step: limit", base, bonus=8, plen=4, limit=7),
        row("step: already at the limit", base, bonus=8, plen=4, limit=6),
        row("step: finished", base, bonus=8, plen=4, fin=1),
        row("step: seam", base + [3], bonus=4, plen=4),
        row("step: the current token alone is no stop", base + [7], bonus=8, plen=4),
    ], T, n=1, cap=48, step=True)
    g["no_table"] = assemble([
        row("S = 0: a limit inside the path", base, [7, 7, 7], 7, limit=8),
        row("S = 0: none", base, [7, 7, 7], 7),
    ], None, n=12, cap=48)
    off = table([[7], [20, 21], [5, -1, 6], [8]], S=6, W=3)
    off[1][0] = 0                                                            # length 0
    off[1][1] = 4                                                            # length > W
    off[0][3, 1] = -9                                                        # a negative id BEHIND the used part: the row stays on
    off[1][4] = -1                                                           # a negative length
    g["rows_off"] = assemble([
        row("turned-off rows: length 0", base, [7, 30], 31),
        row("turned-off rows: length beyond W", base, [20, 21, 30], 31),
        row("turned-off rows: a negative id in the used part", base, [5, -1, 6], 31),
        row("a negative id behind the used part leaves the row on", base, [30, 8, 31], 32),
    ], off, n=12, cap=48, prompts=False)
    rng = np.random.default_rng(4)
    big = [[250]] + [rng.integers(200, 300, size=int(rng.integers(1, 9))).tolist() for _ in range(30)] + [[41, 42, 43, 44, 45, 46, 47, 48]]
    long_text = [60 + i % 30 for i in range(100)]
    g["tree64"] = assemble([
        row("S = 32, W = 8: five history tokens and three emitted ones", long_text + [41, 42, 43, 44, 45], [46, 47, 48, 50], 51, plen=100),
        row("64 nodes, stop at the bonus token e_64", long_text, list(range(300, 363)), 250, plen=100),
        row("64 nodes, an eight-token stop ending at e_64", long_text, list(range(300, 356)) + [41, 42, 43, 44, 45, 46, 47], 48, plen=100),
        row("64 nodes, the limit at index 64", long_text, list(range(300, 363)), 50, plen=100, limit=164),
        row("64 nodes, none", long_text, list(range(300, 363)), 50, plen=100),
        row("64 nodes, clipped at e_63", long_text, list(range(300, 355)) + [41, 42, 43, 44, 45, 46, 47, 48], 50, plen=100),
    ], table(big, S=32, W=8), n=64, cap=200)
    g["tree64_bare"] = assemble([
        row("no prompt_lens, no limits: a stop in the first tokens counts", [3], [4, 20], 21),
        row("no prompt_lens, no limits: none", base, [20, 21], 22),
    ], T, n=64, cap=200, limits=False, prompts=False, max_accept=5)
    return g


def random_case(rng, B=8):
    """A launch over a six-token vocabulary, so that stops and limits fall inside the paths often."""
    n = int(rng.choice([1, 2, 5, 12, 12, 64]))
    max_accept = int(rng.integers((n + 1) // 2, n + 1))
    cap = int(rng.integers(4, 40))
    stops = [rng.integers(0, 6, size=int(rng.integers(1, 4))).tolist() for _ in range(int(rng.integers(1, 5)) if rng.random() < 0.85 else 0)]
    rows = []
    for b in range(B):
        L = int(rng.integers(0, cap + 1))
        m = int(rng.integers(0, max_accept + 1)) if rng.random() < 0.3 else max_accept
        path = rng.integers(0, 6, size=max(m - 1, 0)).tolist()
        rows.append(row(f"random {b}", rng.integers(0, 6, size=L).tolist(), path, int(rng.integers(0, 6)), plen=int(rng.integers(0, L + 2)),
                        limit=int(L + rng.integers(-1, m + 3)) if rng.random() < 0.4 else NO_LIMIT,
                        fin=int(rng.choice([0, 0, 0, 0, 0, 0, 1, 2])), m=m,
                        length=L if rng.random() < 0.9 else int(L + rng.integers(-2 * cap, 2 * cap)),
                        idx=None if rng.random() < 0.5 else rng.integers(-2, n + 2, size=max(m - 1, 0)).tolist()))
    case = assemble(rows, table(stops, S=len(stops) + int(rng.integers(0, 2))) if stops or rng.random() < 0.5 else None, n=n, cap=cap,
                    check_root=int(rng.random() < 0.2), max_accept=max_accept, limits=rng.random() < 0.8, prompts=rng.random() < 0.8,
                    stride=cap + int(rng.integers(0, 5)), fill=0, step=n == 1 and rng.random() < 0.5)
    case["history"] %= 6                                                     # (the filler joins the vocabulary)
    if case["node_tokens"] is not None:
        case["node_tokens"] %= 6
    case["names"] = [f"random: n={n} max_accept={max_accept} cap={cap} row {b}" for b in range(B)]
    return case


def gpu_cases():
    """Everything the GPU test launches: the named launches and 24 random ones."""
    g = named_cases()
    rng = np.random.default_rng(12)
    for i in range(24):
        g[f"random{i}"] = random_case(rng)
    return g
