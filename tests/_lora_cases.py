"""Cases and the float64 oracle of `qs_lora_rows` (include/qserve_amd.h), shared by tests/test_lora_rows_cpu.py and
tests/test_lora_rows_gpu.py; plus synthetic PEFT-named adapters for a model config, shared with the engine tests.

The rule, for row t of T with s = t // rows_per_seq and a = seq_adapter[s] in 0 .. slots-1 (any other a: the row is untouched), for
column n in segment g:
    t_j       = x_scale[t] * sum_k A[a, g r + j, k] * x[t, k]
    out[t, n] = fp16(out[t, n] + scaling[a] * sum_j B[a, n, j] * t_j)
The oracle evaluates it in float64 and returns, next to y, the magnitude M = scaling * sum_j |B| * x_scale * sum_k |A| |x| of the
tolerance  |got - y| <= 2^-11 |y| + 2^-24 + 2 (K + r + 4) 2^-24 M:  the first two terms are the final fp16 rounding (half an ulp of a
normal, half a subnormal step), the last a float32 summation of exact fp16 x int8 products in any order, with the two scalings."""
import numpy as np

SENTINEL_H = np.float16(-1234.0)
SENTINEL_X = np.int8(-77)


def oracle(out, x, x_scale, A, B, scaling, seq_adapter, rows_per_seq, seg_ends):
    """-> (y float64 [T, N], M float64 [T, N], active bool [T])."""
    T, N = out.shape
    slots, r = B.shape[0], B.shape[2]
    y, M, active = out.astype(np.float64), np.zeros((T, N)), np.zeros(T, dtype=bool)
    A64, B64, x64, xs64 = A.astype(np.float64), B.astype(np.float64), x.astype(np.float64), x_scale.astype(np.float64)
    starts = [0] + list(seg_ends[:-1])
    for t in range(T):
        a = int(seq_adapter[t // rows_per_seq])
        if not 0 <= a < slots:
            continue
        active[t] = True
        sc = float(scaling[a])
        for g, (n0, n1) in enumerate(zip(starts, seg_ends)):
            Ag = A64[a, g * r:(g + 1) * r]
            tj = xs64[t] * (Ag @ x64[t])
            y[t, n0:n1] += sc * (B64[a, n0:n1] @ tj)
            M[t, n0:n1] = abs(sc) * (np.abs(B64[a, n0:n1]) @ (xs64[t] * (np.abs(Ag) @ np.abs(x64[t]))))
    return y, M, active


def tolerance(y, M, K, r):
    return 2.0 ** -11 * np.abs(y) + 2.0 ** -24 + 2.0 * (K + r + 4) * 2.0 ** -24 * M


# name -> (T, rows_per_seq, K, N, seg_ends, r, slots, adapters per sequence; None: mixed at random with -1, `slots` and -7 among them).
# T in {1, 3, 64, 130} as the rule's corner sizes (one row, fewer rows than a tile, many one-row tiles, 65-row sequences = five tiles,
# the last of one row) plus T = 36 for rows_per_seq = 12, which divides none of them; K from one wave's share (128) over a partial slice
# (256) and eight slices (4096) to 28 slices (14336, at T = 3); every r; nseg * r = 8 and 24 leave a 16-row MFMA tile partly empty,
# 192 takes three j groups.
SHAPES = {
    "one_row": (1, 1, 128, 64, (64,), 8, 1, [0]),
    "mlp_wide": (3, 1, 14336, 28672, (14336, 28672), 16, 4, [2, -1, 0]),
    "one_seq_r64": (3, 3, 256, 1024, (512, 768, 1024), 64, 1, [0]),
    "step_64": (64, 1, 4096, 1024, (512, 768, 1024), 16, 4, None),
    "two_long_seqs": (130, 65, 256, 1024, (512, 768, 1024), 32, 4, [3, 1]),
    "many_short_seqs": (130, 5, 4096, 64, (64,), 8, 4, None),
    "tree_12_r8": (36, 12, 128, 1024, (512, 768, 1024), 8, 4, [1, -1, 2]),
    "three_j_groups": (130, 65, 128, 1024, (512, 768, 1024), 64, 1, [0, 1]),
}


def make_case(name, seed=0):
    """The tensors of one case, as numpy arrays: `out_store` fp16 [T + 2, N + 8] and `x_store` int8 [T + 2, K + 16] are filled with
    sentinels, the tensors proper are rows 1 .. T, columns 0 .. N-1 / K-1 of them (a guard row on either side, padding behind every
    row)."""
    T, rps, K, N, ends, r, slots, ids = SHAPES[name]
    rng = np.random.default_rng([seed, sorted(SHAPES).index(name)])
    nseq = T // rps
    if ids is None:
        ids = rng.integers(0, slots, size=nseq)
        ids[rng.permutation(nseq)[:3]] = (-1, slots, -7)
    ids = np.asarray(ids, dtype=np.int32)
    assert ids.shape == (nseq,)
    out_store = np.full((T + 2, N + 8), SENTINEL_H, dtype=np.float16)
    x_store = np.full((T + 2, K + 16), SENTINEL_X, dtype=np.int8)
    out_store[1:T + 1, :N] = rng.normal(0.0, 1.0, size=(T, N)).astype(np.float16)
    x_store[1:T + 1, :K] = rng.integers(-128, 128, size=(T, K), dtype=np.int8)
    return dict(name=name, T=T, rows_per_seq=rps, K=K, N=N, seg_ends=tuple(ends), r=r, slots=slots, seq_adapter=ids,
                out_store=out_store, x_store=x_store, x_scale=rng.uniform(0.005, 0.05, size=T).astype(np.float16),
                A=rng.normal(0.0, 0.05, size=(slots, len(ends) * r, K)).astype(np.float16),
                B=rng.normal(0.0, 0.2, size=(slots, N, r)).astype(np.float16),
                scaling=rng.uniform(0.5, 2.0, size=slots).astype(np.float32))


def views(c):
    T, K, N = c["T"], c["K"], c["N"]
    return c["out_store"][1:T + 1, :N], c["x_store"][1:T + 1, :K]


def case_oracle(c):
    out, x = views(c)
    return oracle(out, x, c["x_scale"], c["A"], c["B"], c["scaling"], c["seq_adapter"], c["rows_per_seq"], c["seg_ends"])


# ---- synthetic adapters under PEFT's names ------------------------------------------------------------------------------------------
PREFIX = "base_model.model.model.layers."
MODULES = (("self_attn", "q"), ("self_attn", "k"), ("self_attn", "v"), ("self_attn", "o"), ("mlp", "gate"), ("mlp", "up"), ("mlp", "down"))


def module_shapes(cfg):
    """module -> (K, N) of the separate projections of a layer (heads are 128 wide)."""
    hid, H, Hkv, inter = cfg["hidden"], cfg["heads"], cfg["kv_heads"], cfg["inter"]
    return dict(q=(hid, H * 128), k=(hid, Hkv * 128), v=(hid, Hkv * 128), o=(H * 128, hid), gate=(hid, inter), up=(hid, inter),
                down=(inter, hid))


def peft_adapter(cfg, rank, seed, std=0.05, skip=()):
    """{name: torch fp16 tensor} for every layer and module of `cfg` but those in `skip` ((layer, module) pairs)."""
    import torch
    gen = torch.Generator().manual_seed(seed)
    shapes, d = module_shapes(cfg), {}
    for li in range(cfg["layers"]):
        for block, mod in MODULES:
            if (li, mod) in skip:
                continue
            K, N = shapes[mod]
            d[f"{PREFIX}{li}.{block}.{mod}_proj.lora_A.weight"] = (torch.randn((rank, K), generator=gen) * std).half()
            d[f"{PREFIX}{li}.{block}.{mod}_proj.lora_B.weight"] = (torch.randn((N, rank), generator=gen) * std).half()
    return d
