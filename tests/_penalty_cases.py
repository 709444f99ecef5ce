"""The rule of `qs_penalize_rows` (include/qserve_amd.h) twice - a float64 oracle written as a straight loop over each row's context,
and a numpy float32 restatement that performs the kernel's operations one by one (bit-equal to the kernel) - and the cases the CPU and
GPU tests share.  A case is a dict: logits fp16 [B * n_nodes, stride] (the padding behind n included), n, history int32 [B, hist_stride],
cap, lengths int32 [B], prompt_lens int32 [B] or None, node_tokens int64 [B, n_nodes] or None, parents (list) or None, n_nodes, and rep /
freq / pres: a float each or a float32 array [B]."""
import numpy as np

NEG_INF = -np.inf
CANARY = 0x7E5A                     # a NaN pattern no arithmetic produces: what must not be written is filled with it


def path_nodes(parents, i):
    """The nodes != 0 on the path root -> i, in path order; a node whose parent entry is not in 0 .. j - 1 hangs off the root."""
    out, j = [], i
    while j > 0:
        out.append(j)
        a = int(parents[j])
        j = a if 0 <= a < j else 0
    return out[::-1]


def param(case, name, b):
    v = case[name]
    return np.float32(v[b] if isinstance(v, np.ndarray) else v)


def context(case, b, i):
    """[(token, generated)] of row b * n_nodes + i: the clamped history, then the path's tokens (all generated)."""
    L = min(max(int(case["lengths"][b]), 0), case["cap"])
    P = 0 if case["prompt_lens"] is None else int(case["prompt_lens"][b])
    ctx = [(int(case["history"][b, p]), p >= P) for p in range(L)]
    if case["node_tokens"] is not None:
        ctx += [(int(case["node_tokens"][b, j]), True) for j in path_nodes(case["parents"], i)]
    return ctx


def neutral(case, b):
    return param(case, "rep", b) == 1 and param(case, "freq", b) == 0 and param(case, "pres", b) == 0


def oracle64(case):
    """-> one dict {token id: float64 value} per row: the ids the rule edits and their exact penalised value (-inf logits and neutral
    sequences excluded - they are not written).  A straight loop over the context."""
    rows = []
    n = case["n"]
    for b in range(case["history"].shape[0]):
        rep, freq, pres = (float(param(case, k, b)) for k in ("rep", "freq", "pres"))
        for i in range(case["n_nodes"]):
            out = {}
            if not neutral(case, b):
                c_all, c_gen = {}, {}
                for t, gen in context(case, b, i):
                    if 0 <= t < n:
                        c_all[t] = c_all.get(t, 0) + 1
                        c_gen[t] = c_gen.get(t, 0) + (1 if gen else 0)
                row = case["logits"][b * case["n_nodes"] + i]
                for t in c_all:
                    x = float(row[t])
                    if x == NEG_INF:
                        continue
                    x = x / rep if x > 0 else x * rep
                    x = x - (freq * c_gen[t] + (pres if c_gen[t] > 0 else 0.0))
                    out[t] = x
            rows.append(out)
    return rows


def dense_counts(case):
    """(c_all, c_gen) int64 [rows, n] by np.bincount (the restatement's counting: no loop shared with the oracle)."""
    n, nn = case["n"], case["n_nodes"]
    B = case["history"].shape[0]
    c_all, c_gen = np.zeros((B * nn, n), np.int64), np.zeros((B * nn, n), np.int64)
    for b in range(B):
        L = min(max(int(case["lengths"][b]), 0), case["cap"])
        P = 0 if case["prompt_lens"] is None else int(case["prompt_lens"][b])
        h = case["history"][b, :L].astype(np.int64)
        ok = (h >= 0) & (h < n)
        gen = np.arange(L) >= P
        base_all, base_gen = np.bincount(h[ok], minlength=n), np.bincount(h[ok & gen], minlength=n)
        for i in range(nn):
            r = b * nn + i
            c_all[r], c_gen[r] = base_all, base_gen
            if case["node_tokens"] is not None:
                t = case["node_tokens"][b, path_nodes(case["parents"], i)].astype(np.int64)
                t = t[(t >= 0) & (t < n)]
                extra = np.bincount(t, minlength=n)
                c_all[r] += extra
                c_gen[r] += extra
    return c_all, c_gen


def restate32(case):
    """The rows after the kernel, as uint16 bits [rows, stride]: float32 operations, each rounded on its own, then fp16 (RNE)."""
    n, nn = case["n"], case["n_nodes"]
    c_all, c_gen = dense_counts(case)
    out = case["logits"].copy()
    f32 = np.float32
    with np.errstate(all="ignore"):
        for r in range(out.shape[0]):
            b = r // nn
            if neutral(case, b):
                continue
            rep, freq, pres = (param(case, k, b) for k in ("rep", "freq", "pres"))
            x = case["logits"][r, :n].astype(f32)
            y = np.where(x > 0, x / rep, x * rep).astype(f32)
            pen = (freq * c_gen[r].astype(f32)).astype(f32)
            pen = (pen + np.where(c_gen[r] > 0, pres, f32(0))).astype(f32)
            y = (y - pen).astype(f32)
            edit = (c_all[r] > 0) & (x != NEG_INF)
            out[r, :n] = np.where(edit, y.astype(np.float16), case["logits"][r, :n])
    return out.view(np.uint16)


def ordered(bits):
    """fp16 bits -> integers that order like the values, neighbours one apart (-0 and +0 coincide)."""
    b = np.asarray(bits, dtype=np.uint16).astype(np.int64)
    return np.where(b & 0x8000, -(b & 0x7FFF), b)


def check_against_oracle(case, got_bits):
    """`got_bits` uint16 [rows, stride] against the float64 oracle: every edited id within one fp16 ulp of the oracle's value rounded
    to fp16, every other element (ids outside the context, -inf logits, the padding, neutral rows) bit-identical to the input.
    -> the number of edited logits."""
    src = case["logits"].view(np.uint16)
    edited = 0
    for r, want in enumerate(oracle64(case)):
        untouched = np.ones(src.shape[1], bool)
        if want:
            ids = np.fromiter(want.keys(), np.int64, len(want))
            with np.errstate(over="ignore"):
                ref = np.array([want[int(t)] for t in ids], np.float64).astype(np.float16)
            d = np.abs(ordered(got_bits[r, ids]) - ordered(ref.view(np.uint16)))
            assert d.max() <= 1, f"row {r}: id {int(ids[d.argmax()])} is {int(d.max())} fp16 ulps from the oracle"
            untouched[ids] = False
            edited += len(want)
        assert np.array_equal(got_bits[r, untouched], src[r, untouched]), f"row {r}: an element outside the rule's edits was written"
    return edited


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
def _logits(rng, rows, n, stride):
    """Positive, negative, zero and -inf logits; the padding behind n holds the canary."""
    x = (rng.standard_normal((rows, stride)) * 3.0).astype(np.float16)
    x[rng.random((rows, stride)) < 0.05] = 0.0
    x[rng.random((rows, stride)) < 0.05] = NEG_INF
    x.view(np.uint16)[:, n:] = CANARY
    return x


def _case(rng, n, stride, history, cap, lengths, prompt_lens, node_tokens, parents, rep, freq, pres):
    B = history.shape[0]
    nn = 1 if parents is None else len(parents)
    arr = lambda v: np.asarray(v, np.float32) if isinstance(v, (list, tuple)) else float(v)   # noqa: E731
    case = dict(n=n, n_nodes=nn, history=np.ascontiguousarray(history, dtype=np.int32), cap=cap, lengths=np.asarray(lengths, np.int32),
                prompt_lens=None if prompt_lens is None else np.asarray(prompt_lens, np.int32),
                node_tokens=None if node_tokens is None else np.asarray(node_tokens, np.int64), parents=parents,
                rep=arr(rep), freq=arr(freq), pres=arr(pres), logits=_logits(rng, B * nn, n, stride))
    for b in range(B):                                   # neutral rows must not be written: canaries all over
        if neutral(case, b):
            case["logits"].view(np.uint16)[b * nn:(b + 1) * nn] = CANARY
    return case


def chain(n):
    return [-1] + list(range(n - 1))


BRANCHING = [-1, 0, 0, 1, 1, 2, 0]
MALFORMED = [-1, 0, 5, 1, -3, 2, 4, 99, 7]             # nodes 2, 4, 7 hang off the root; 6 hangs off 4, 8 off 7
I31 = 2 ** 31 - 1


def gpu_cases():
    """name -> case: the smallest shapes at which the kernel can go wrong (tests/test_penalize_rows_gpu.py lists what each one plants)."""
    rng = np.random.default_rng(20)
    cases = {}
    # n = 8, the minimum; n_nodes = 1 without node_tokens; lengths 0, 1, cap, > cap; prompt_lens 0, = L, > L; ignored ids
    h = rng.integers(0, 8, size=(4, 16))
    h[2, :6] = [-1, 8, I31, 0, 7, -2 ** 31]
    cases["min_vocab"] = _case(rng, 8, 8, h, 16, [0, 1, 16, 40], [0, 1, 99, 5], None, None, 1.3, 0.2, 0.4)
    # two slices, the second partial, padding behind n; slice-edge ids; siblings with different tokens under a large penalty;
    # per-sequence parameters with a neutral sequence between two penalised ones; rep < 1, negative freq / pres; prompt_lens null
    n = 33000
    h = rng.integers(0, n, size=(3, 96))
    h[:, :8] = [0, 32767, 32768, n - 1, -1, n, I31, 32768]
    nodes = rng.integers(0, n, size=(3, len(BRANCHING)))
    nodes[0] = [5, 11111, 22222, 32767, 32768, n - 1, 0]               # every node another token: a leak moves a logit by ~50
    nodes[2] = [5, n, -1, I31, 1 << 40, 22222, 22222]                   # ignored ids on the paths (n itself: a leak lands in the
    #                                                                     padding's canaries); 5 and 6 equal, on different paths
    cases["two_slices"] = _case(rng, n, 33008, h, 96, [96, 50, 95], None, nodes, BRANCHING, [1.7, 1.0, 0.6], [0.3, 0.0, -0.25],
                                [50.0, 0.0, -2.0])
    # the full vocabulary once; padded, unaligned history rows (row stride 515); per-sequence repetition only
    n = 128256
    h = rng.integers(0, n, size=(2, 515))
    h[:, 300:320] = h[:, 100:120]                                       # repeats
    nodes = np.stack([h[0, [0, 100, 101, 7]], rng.integers(0, n, size=4)])
    cases["big_vocab"] = _case(rng, n, n, h, 512, [400, 513], [100, 0], nodes, [-1, 0, 1, 0], [1.2, 0.9], 0.1, 0.5)
    # a 64-node chain carrying one token: multiplicity 63, on a base count of zero (sequence 0) and of three (sequence 1)
    h = rng.integers(0, 30, size=(2, 24))
    h[0][h[0] == 33] = 1
    h[1, 3:6] = 33
    cases["chain64"] = _case(rng, 40, 40, h, 24, [24, 20], [4, 30], np.full((2, 64), 33), chain(64), 1.1, 0.05, 0.3)
    # malformed parent entries
    h = rng.integers(0, 24, size=(2, 12))
    cases["malformed"] = _case(rng, 24, 24, h, 12, [12, 7], [3, 3], rng.integers(0, 24, size=(2, len(MALFORMED))), MALFORMED, 0.8, 0.5, -0.7)
    # one id 40 000 times at cap = 40 000: counts above 2^15 in both halves; the node repeats it once more
    h = np.full((1, 40000), 9)
    cases["count40000"] = _case(rng, 16, 16, h, 40000, [40000], [100], [[3, 9]], [-1, 0], 1.5, 0.01, 1.0)
    return cases


def random_case(rng):
    """A small random case for the CPU agreement tests: any tree (malformed entries included), ragged lengths, ignored ids."""
    n = int(rng.choice([8, 12, 40]))
    B, cap = int(rng.integers(1, 4)), int(rng.integers(1, 30))
    nn = int(rng.integers(1, 10))
    par = [-1] + [int(rng.integers(-1, i + 1)) for i in range(1, nn)]
    h = rng.integers(-1, n + 1, size=(B, cap))
    nodes = rng.integers(-1, n + 1, size=(B, nn)) if rng.random() < 0.8 else None
    pick = lambda vals: [float(rng.choice(vals)) for _ in range(B)] if rng.random() < 0.5 else float(rng.choice(vals))   # noqa: E731
    return _case(rng, n, n + int(rng.choice([0, 8])) if n % 8 == 0 else n + (8 - n % 8), h, cap, rng.integers(-1, cap + 3, size=B),
                 None if rng.random() < 0.3 else rng.integers(0, cap + 2, size=B), nodes, par if nodes is not None or nn > 1 else None,
                 pick([1.0, 1.3, 0.7, 2.0]), pick([0.0, 0.1, -0.3, 1.5]), pick([0.0, 0.4, -1.0]))
