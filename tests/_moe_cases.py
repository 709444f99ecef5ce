"""Numpy restatements of the mixture-of-experts rules of include/qserve_amd.h (`qs_moe_route`, `qs_w4a8_per_*_moe_gemm`,
`qs_moe_combine`) and the case table the CPU and GPU tests share.  Nothing here imports the product."""
import numpy as np

# ---- routing ----------------------------------------------------------------------------------------------------------------------


def route_ref(logits, k):
    """logits fp16 [T, E] -> (expert_ids int32 [T, k], weights float64 [T, k], expert_offsets int32 [E + 1], pair_token int32 [T k],
    pair_pos int32 [T, k]).  Selection: the k largest logits by (value descending, expert index ascending), compared as the fp16 values
    they are.  Weights: softmax over the k chosen logits, here in float64 (the kernel's float32 value is held to a derived bound of it).
    Sort: stable by expert - inside an expert the pairs keep their (t, j) order."""
    logits = np.asarray(logits, np.float16)
    T, E = logits.shape
    v = logits.astype(np.float64)
    order = np.argsort(-v, axis=1, kind="stable")[:, :k]            # stable on -v: value descending, index ascending
    ids = order.astype(np.int32)
    chosen = np.take_along_axis(v, order, axis=1)
    e = np.exp(chosen - chosen[:, :1])
    w = e / e.sum(axis=1, keepdims=True)
    flat = ids.reshape(-1)
    perm = np.argsort(flat, kind="stable")                          # sorted position -> pair
    offsets = np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=E))]).astype(np.int32)
    pair_token = (perm // k).astype(np.int32)
    pair_pos = np.empty(T * k, np.int32)
    pair_pos[perm] = np.arange(T * k, dtype=np.int32)
    return ids, w, offsets, pair_token, pair_pos.reshape(T, k)


def route_weight_bound(logits, ids, w64, exp_ulps=1.0):
    """|kernel float32 weight - float64 softmax| <= this, elementwise [T, k], for the kernel's op sequence
        e_j = expf(float(l_j) - float(l_0));  s = ((e_0 + e_1) + ...) + e_{k-1};  w_j = e_j / s.
    With u = 2^-24 (half an ulp, relative) and x_j = l_j - l_0 <= 0:
      * the subtraction of two fp16 values is rounded once in float32: |dx| <= u |x_j|, which moves e^x_j by a factor e^dx, relative
        error <= u |x_j| (1 + tiny);
      * expf: `exp_ulps` ulps, relative <= exp_ulps * 2u.  The figure is AMD's: the HIP math API documentation (ROCm docs, "HIP math API",
        single precision table) lists expf with a maximum error of 1 ULP; the device library ships as bitcode without that page, so it
        is quoted, not read from a file of the toolchain;
      * so every e_j carries d = 2u exp_ulps + u max|x|; the k-term sum of positive terms keeps the worst relative error of its terms and
        adds u per addition: d + (k - 1) u;
      * the IEEE division adds u.
    Relative error of w_j <= 2 d + k u, first order; the second-order terms are covered by the factor 1.001.  A quotient may be
    subnormal: absolute floor 2^-126."""
    lg = np.asarray(logits, np.float16).astype(np.float64)
    k = ids.shape[1]
    chosen = np.take_along_axis(lg, ids.astype(np.int64), axis=1)
    xmax = np.abs(chosen - chosen[:, :1]).max(axis=1, keepdims=True)
    u = 2.0 ** -24
    d = 2 * u * exp_ulps + u * xmax
    return w64 * (2 * d + k * u) * 1.001 + 2.0 ** -126


def _rows(rng, T, E, scale=2.0):
    return (rng.standard_normal((T, E)) * scale).astype(np.float16)


REQUIRED_T = (1, 3, 64, 130)
REQUIRED_EK = ((1, 1), (4, 2), (8, 2), (8, 8), (64, 8))
EXTRA_T = (300, 2500)          # beyond the one-launch path of the kernel (T > 256; T k > 2048)


def route_cases():
    """[(name, logits fp16 [T, E], k)]: the table both tests walk.  Every T of REQUIRED_T with every (E, k) of REQUIRED_EK on random rows;
    rows with all logits equal; ties across the k-th place; an expert that receives nothing; every pair on one expert; two sizes that take
    the multi-launch path."""
    rng = np.random.default_rng(20)
    cases = []
    for T in REQUIRED_T:
        for E, k in REQUIRED_EK:
            cases.append((f"random-T{T}-E{E}-k{k}", _rows(rng, T, E), k))
    for E, k in REQUIRED_EK:
        lg = _rows(rng, 5, E)
        lg[1, :] = np.float16(0.75)                                  # a row with all logits equal
        lg[3, :] = np.float16(-3.0)
        cases.append((f"all-equal-E{E}-k{k}", lg, k))
    for E, k in ((4, 2), (8, 2), (64, 8)):
        lg = _rows(rng, 6, E)
        for t in range(6):                                           # the k-th largest value stands in k - 1 .. k + 1 places and more
            top = np.sort(lg[t].astype(np.float32))[::-1][k - 1]
            where = rng.choice(E, size=min(E, k + 2), replace=False)
            lg[t, where] = np.float16(top)
        cases.append((f"ties-at-kth-E{E}-k{k}", lg, k))
    lg = _rows(rng, 64, 8)
    lg[:, 5] = np.float16(-30.0)                                     # expert 5 receives nothing
    cases.append(("empty-expert-E8-k2", lg, 2))
    lg = _rows(rng, 64, 8, scale=0.5)
    lg[:, 2] = np.float16(9.0)                                       # every token's first pair on expert 2 ...
    cases.append(("one-expert-first-E8-k2", lg, 2))
    cases.append(("one-expert-all-E8-k1", lg.copy(), 1))             # ... and with k = 1 every pair
    cases.append(("one-expert-all-E1-k1", _rows(rng, 130, 1), 1))
    for T in EXTRA_T:
        cases.append((f"random-T{T}-E8-k2", _rows(rng, T, 8), 2))
    cases.append(("random-T300-E64-k8", _rows(rng, 300, 64), 8))
    return cases


# ---- combine ------------------------------------------------------------------------------------------------------------------------


def combine_ref(y, weights, pair_pos):
    """out[t] = half(sum_j weights[t, j] * float(y[pair_pos[t, j]])): float32, j ascending, the first product alone, every multiply and add
    rounded on its own, one rounding to fp16."""
    y = np.asarray(y, np.float16).astype(np.float32)
    w = np.asarray(weights, np.float32)
    T, k = w.shape
    acc = None
    for j in range(k):
        term = (w[:, j:j + 1] * y[pair_pos[:, j]]).astype(np.float32)
        acc = term if acc is None else (acc + term).astype(np.float32)
    return acc.astype(np.float16)


# ---- the grouped GEMM's row plans -------------------------------------------------------------------------------------------------------

# rows per expert for every m-tile count the planner returns: 0, 1, 15, 16, 17, 16 mt, 16 mt + 1 (and what lifts the mean into the
# planner's band: ceil(P / E) <= 16 -> 1, <= 32 -> 2, else 4)
ROWS_PER_EXPERT = {1: [0, 1, 15, 16, 17, 16, 17], 2: [0, 1, 15, 16, 17, 32, 33], 4: [0, 1, 15, 16, 17, 64, 65, 120]}


def true_row_blocks(counts, mt):
    return sum((c + 16 * mt - 1) // (16 * mt) for c in counts)


def plan_ref(P, E, N, K):
    """The planner of csrc/moe_plan.h restated: (mt, waves, row blocks launched, units)."""
    avg = -(-P // E)
    mt = 1 if avg <= 16 else 2 if avg <= 32 else 4
    steps = K // 128
    nw = 8 if steps >= 16 and mt <= 2 else 4 if steps >= 3 else 2 if steps >= 2 else 1
    blocks = 0 if P <= 0 else -(-P // (16 * mt)) + E - 1
    return mt, nw, blocks, N // 64
