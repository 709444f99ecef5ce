"""Mixture of experts on the CPU: the numpy routing restatement of tests/_moe_cases.py against an independent torch statement in float64,
the case table's own coverage, the planner `qs_moe_gemm_plan` against a committed table and against the true block counts, every
argument rule of the four entries (they answer before any device call), and `loader.load_mixtral_w4a8` against slices written by hand."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import _moe_cases as K

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = K.route_cases()


@pytest.fixture(scope="module")
def lib(built_lib):
    from qserve_amd._lib import lib
    return lib


# ---- the routing restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,logits,k", CASES, ids=[c[0] for c in CASES])
def test_route_restatement_against_torch(name, logits, k):
    """torch.topk for the values, a stable descending sort for the ids (value descending, index ascending), softmax over ALL experts
    renormalised over the chosen ones (the Mixtral statement), argsort(stable) for the expert sort - float64 throughout."""
    ids, w, offsets, pair_token, pair_pos = K.route_ref(logits, k)
    T, E = logits.shape
    lg = torch.from_numpy(logits.astype(np.float64))
    vals, order = torch.sort(lg, dim=1, descending=True, stable=True)
    assert torch.equal(torch.topk(lg, k, dim=1).values, vals[:, :k])
    want_ids = order[:, :k]
    assert np.array_equal(ids, want_ids.numpy().astype(np.int32))
    for t in range(T):                                               # the order, spelled out: no pair (value, index) out of place
        key = [(-float(lg[t, i]), int(i)) for i in ids[t]]
        assert key == sorted(key) and len(set(ids[t].tolist())) == k
        rest = [(-float(lg[t, i]), i) for i in range(E) if i not in set(ids[t].tolist())]
        assert not rest or max(key) < min(rest)
    full = torch.softmax(lg, dim=1).gather(1, want_ids)
    want_w = full / full.sum(dim=1, keepdim=True)
    assert np.allclose(w, want_w.numpy(), rtol=1e-12, atol=1e-300)
    assert np.allclose(w.sum(axis=1), 1.0, rtol=1e-12)
    flat = want_ids.reshape(-1)
    perm = torch.argsort(flat, stable=True)
    assert np.array_equal(pair_token, (perm // k).numpy().astype(np.int32))
    assert np.array_equal(pair_pos.reshape(-1)[perm.numpy()], np.arange(T * k))
    counts = torch.bincount(flat, minlength=E).numpy()
    assert offsets[0] == 0 and offsets[E] == T * k and np.array_equal(np.diff(offsets), counts)
    for e in range(E):                                               # stable: inside an expert the pairs are ordered by (t, j)
        seg = perm.numpy()[offsets[e]:offsets[e + 1]]
        assert (np.diff(seg) > 0).all() and (flat.numpy()[seg] == e).all()


def test_the_case_table_covers_what_it_says():
    seen = {(lg.shape[0], lg.shape[1], k) for name, lg, k in CASES if name.startswith("random")}
    assert seen >= {(T, E, k) for T in K.REQUIRED_T for E, k in K.REQUIRED_EK}
    by_name = {name: (lg, k) for name, lg, k in CASES}
    assert any((lg == lg[:, :1]).all(axis=1).any() for name, (lg, k) in by_name.items() if name.startswith("all-equal"))
    for name, (lg, k) in by_name.items():
        if name.startswith("ties-at-kth"):
            v = np.sort(lg.astype(np.float32), axis=1)[:, ::-1]
            assert ((lg.astype(np.float32) == v[:, k - 1:k]).sum(axis=1) >= 2).all(), name     # the k-th value stands in several places
            assert (v[:, k - 1] == v[:, k]).any() if lg.shape[1] > k else True, name             # ... on both sides of the cut
    lg, k = by_name["empty-expert-E8-k2"]
    assert np.diff(K.route_ref(lg, k)[2])[5] == 0
    lg, k = by_name["one-expert-all-E8-k1"]
    assert np.diff(K.route_ref(lg, k)[2]).tolist() == [0, 0, lg.shape[0], 0, 0, 0, 0, 0]
    assert any(lg.shape[0] > 256 for name, lg, k in CASES) and any(lg.shape[0] * k > 2048 for name, lg, k in CASES)


# ---- the planner ------------------------------------------------------------------------------------------------------------------------
def _plan(lib, P, E, N, Kk):
    plan = (ctypes.c_int * 4)()
    assert lib.qs_moe_gemm_plan(P, E, N, Kk, plan) == 0, lib.qs_last_error()
    return list(plan)


def test_plan_table(lib):
    """qs_moe_gemm_plan against the committed table (tests/golden/moe_plan_table.json: [[P, E, N, K], [mt, waves, row blocks, units]])
    and against the restated rule."""
    table = json.load(open(os.path.join(HERE, "golden", "moe_plan_table.json")))["plans"]
    assert len(table) >= 40 and {row[1][0] for row in table} == {1, 2, 4} and {row[1][1] for row in table} == {1, 2, 4, 8}
    for (P, E, N, Kk), want in table:
        assert _plan(lib, P, E, N, Kk) == want, (P, E, N, Kk)
        assert list(K.plan_ref(P, E, N, Kk)) == want, (P, E, N, Kk)


def test_grid_bound_covers_every_routing(lib):
    """The row blocks launched are at least the blocks any routing needs - the table's shapes, the row plans of the GPU test, the worst
    case (E - 1 single rows, the rest on one expert) and random count vectors."""
    rng = np.random.default_rng(3)
    for mt, counts in K.ROWS_PER_EXPERT.items():
        P, E = sum(counts), len(counts)
        plan = _plan(lib, P, E, 64, 128)
        assert plan[0] == mt, (mt, plan)
        assert plan[2] >= K.true_row_blocks(counts, mt)
    for P, E in [(1, 1), (2, 8), (8, 8), (16, 8), (128, 8), (130, 8), (1040, 64), (4096, 8), (131072, 8), (131072, 64), (63, 64), (64, 64)]:
        mt, _, blocks, _ = _plan(lib, P, E, 256, 512)
        worst = [1] * min(E - 1, P - 1) + [P - min(E - 1, P - 1)]
        assert blocks >= K.true_row_blocks(worst, mt), (P, E)
        assert blocks == -(-P // (16 * mt)) + E - 1
        for _ in range(50):
            cuts = np.sort(rng.integers(0, P + 1, size=E - 1))
            counts = np.diff(np.concatenate([[0], cuts, [P]])).tolist()
            assert blocks >= K.true_row_blocks(counts, mt), (P, E, counts)


# ---- argument rules: every one answers before any device call (no GPU here) ---------------------------------------------------------------
A16 = 4096          # a 16-byte aligned fake address


def _err(lib):
    return lib.qs_last_error().decode()


def test_route_argument_rules(lib):
    ok = dict(logits=A16, stride=8, T=4, E=8, k=2, ids=A16, w=A16, offs=A16, ptok=A16, ppos=A16, ws=A16, wsb=64)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.qs_moe_route(a["logits"], a["stride"], a["T"], a["E"], a["k"], a["ids"], a["w"], a["offs"], a["ptok"], a["ppos"], a["ws"],
                                a["wsb"], None)

    for kw, word in ((dict(E=65), "experts"), (dict(E=0), "experts"), (dict(k=9, E=16, stride=16), "k=9"), (dict(k=3, E=2), "k=3"),
                     (dict(k=0), "k=0"), (dict(T=-1), "T=-1"), (dict(T=(1 << 24) + 1, k=1), "T="), (dict(stride=7), "stride"),
                     (dict(logits=0), "null"), (dict(ids=0), "null"), (dict(w=0), "null"), (dict(offs=0), "null"), (dict(ptok=0), "null"),
                     (dict(ppos=0), "null"), (dict(ws=0), "null"), (dict(logits=A16 + 1), "aligned"), (dict(ids=A16 + 2), "aligned"),
                     (dict(w=A16 + 2), "aligned"), (dict(ppos=A16 + 1), "aligned"),
                     (dict(T=2000, wsb=64), "workspace")):
        assert call(**kw) == -1 and word in _err(lib), (kw, _err(lib))
    assert lib.qs_moe_route_workspace(4, 8, 2) == 16 and lib.qs_moe_route_workspace(2000, 8, 2) == 4 * 8 * 4
    assert lib.qs_moe_route_workspace(4, 65, 2) == -1 and lib.qs_moe_route_workspace(4, 4, 5) == -1


@pytest.mark.parametrize("per_group", [False, True])
def test_grouped_gemm_argument_rules(lib, per_group):
    ok = dict(x=A16, xs=256, xr=16, src=A16, offs=A16, qw=A16, z=A16, s8=A16, ws=A16, asc=A16, wz=A16, asum=A16, out=A16, os=64, P=16, E=8, N=64,
              K=256)

    def call(**kw):
        a = dict(ok, **kw)
        if per_group:
            return lib.qs_w4a8_per_group_moe_gemm(a["x"], a["xs"], a["xr"], a["src"], a["offs"], a["qw"], a["z"], a["s8"], a["ws"], a["asc"],
                                                  a["out"], a["os"], a["P"], a["E"], a["N"], a["K"], None)
        return lib.qs_w4a8_per_chn_moe_gemm(a["x"], a["xs"], a["xr"], a["src"], a["offs"], a["qw"], a["ws"], a["asc"], a["wz"], a["asum"],
                                            a["out"], a["os"], a["P"], a["E"], a["N"], a["K"], None)

    rules = [(dict(E=65), "experts"), (dict(E=0), "experts"), (dict(N=96, os=96), "multiple of 64"), (dict(K=192), "multiple of 128"),
             (dict(P=-1), "P=-1"), (dict(P=(1 << 21) + 1), "P="), (dict(x=0), "null"), (dict(offs=0), "null"), (dict(qw=0), "null"),
             (dict(ws=0), "null"), (dict(asc=0), "null"), (dict(out=0), "null"), (dict(xs=255), "stride"), (dict(xs=128), "stride"),
             (dict(os=60), "stride"), (dict(os=68), "stride"), (dict(xr=0), "x_rows"), (dict(src=0, xr=15), "x_rows"),
             (dict(x=A16 + 8), "aligned"), (dict(out=A16 + 8), "aligned"), (dict(qw=A16 + 4), "aligned"), (dict(ws=A16 + 4), "aligned"),
             (dict(offs=A16 + 2), "aligned"), (dict(src=A16 + 2), "aligned"), (dict(asc=A16 + 1), "aligned")]
    rules += [(dict(z=0), "null"), (dict(s8=0), "null"), (dict(z=A16 + 2), "aligned")] if per_group else \
        [(dict(wz=0), "null"), (dict(asum=0), "null"), (dict(wz=A16 + 4), "aligned"), (dict(asum=A16 + 1), "aligned")]
    for kw, word in rules:
        assert call(**kw) == -1 and word in _err(lib), (kw, _err(lib))
    assert call(P=0) == 0                                            # an empty call: no launch
    plan = (ctypes.c_int * 4)()
    assert lib.qs_moe_gemm_plan(16, 65, 64, 128, plan) == -1 and lib.qs_moe_gemm_plan(16, 8, 100, 128, plan) == -1
    assert lib.qs_moe_gemm_plan(16, 8, 64, 100, plan) == -1 and lib.qs_moe_gemm_plan(16, 8, 64, 128, None) == -1


def test_combine_argument_rules(lib):
    ok = dict(out=A16, os=64, y=A16, ys=64, w=A16, pp=A16, T=4, k=2, N=64)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.qs_moe_combine(a["out"], a["os"], a["y"], a["ys"], a["w"], a["pp"], a["T"], a["k"], a["N"], None)

    for kw, word in ((dict(k=0), "k=0"), (dict(k=9), "k=9"), (dict(T=-1), "T=-1"), (dict(N=96, os=96, ys=96), "multiple of 64"),
                     (dict(N=0), "N=0"), (dict(out=0), "null"), (dict(y=0), "null"), (dict(w=0), "null"), (dict(pp=0), "null"),
                     (dict(os=60), "stride"), (dict(os=68), "stride"), (dict(ys=32), "stride"), (dict(ys=70), "stride"),
                     (dict(out=A16 + 8), "aligned"), (dict(y=A16 + 2), "aligned"), (dict(w=A16 + 2), "aligned"), (dict(pp=A16 + 1), "aligned")):
        assert call(**kw) == -1 and word in _err(lib), (kw, _err(lib))
    assert call(T=0) == 0


# ---- the loader ---------------------------------------------------------------------------------------------------------------------------
CFG = dict(name="moe-test", hidden=256, heads=2, kv_heads=1, inter=128, layers=2, vocab=64, rope_theta=1e4, eps=1e-5, experts=3,
           experts_per_token=2)


def _packed(rng, n, k, group_size):
    """One projection packed with oracle.w4a8, under the checkpoint's tensor names."""
    from oracle import w4a8
    q = rng.integers(0, 16, (n, k), dtype=np.uint8)
    s1 = rng.uniform(0.002, 0.02, n).astype(np.float16)
    if group_size == -1:
        qweight, wscales, w_szs = w4a8.pack_per_channel(q, rng.integers(0, 16, (n,), dtype=np.uint8), s1)
        d = dict(qweight=qweight, s1_scales=wscales, s1_szeros=w_szs)
    else:
        z = rng.integers(0, 16, (n, k // 128)).astype(np.int32)
        s2 = rng.integers(1, 9, (n, k // 128)).astype(np.int32)
        qweight, wscales, s2_scales, s2_zeros = w4a8.pack_per_group(q.astype(np.int32), z, s2, s1)
        d = dict(qweight=qweight, s1_scales=wscales, s2_scales=s2_scales, s2_zeros=s2_zeros)
    return {name: torch.from_numpy(np.ascontiguousarray(t)) for name, t in d.items()}


@pytest.mark.parametrize("group_size", [-1, 128])
def test_load_mixtral_against_hand_written_slices(built_lib, group_size):
    from qserve_amd import loader
    rng = np.random.default_rng(5)
    hid, I, E = CFG["hidden"], CFG["inter"], CFG["experts"]
    state, src = {}, {}
    for li in range(CFG["layers"]):
        p = f"model.layers.{li}."
        for name, (n, k) in dict(q=(256, hid), k=(128, hid), v=(128, hid), o=(hid, 256)).items():
            src[li, name] = _packed(rng, n, k, group_size)
            state.update({f"{p}self_attn.{name}_proj.{t}": v for t, v in src[li, name].items()})
        state[p + "block_sparse_moe.gate.weight"] = torch.from_numpy(rng.standard_normal((E, hid)).astype(np.float32))
        for e in range(E):
            for name, (n, k) in dict(w1=(I, hid), w3=(I, hid), w2=(hid, I)).items():
                src[li, e, name] = _packed(rng, n, k, group_size)
                state.update({f"{p}block_sparse_moe.experts.{e}.{name}.{t}": v for t, v in src[li, e, name].items()})
        state[p + "input_layernorm.weight"] = torch.full((hid,), 3.0)
    state["model.embed_tokens.weight"] = torch.from_numpy(rng.standard_normal((64, hid)).astype(np.float32))
    state["lm_head.weight"] = torch.from_numpy(rng.standard_normal((64, hid)).astype(np.float32))
    out = loader.load_mixtral_w4a8(state, CFG, group_size=group_size)
    llama_like = loader.load_llama_w4a8({k.replace("block_sparse_moe.experts.0.w1", "mlp.gate_proj").replace(
        "block_sparse_moe.experts.0.w3", "mlp.up_proj").replace("block_sparse_moe.experts.0.w2", "mlp.down_proj"): v for k, v in state.items()},
        CFG, group_size=group_size)
    assert len(out["layers"]) == 2 and out["embed"].dtype == torch.float16 and tuple(out["lm_head"].shape) == (64, hid)
    assert torch.equal(out["norm"], torch.ones(hid, dtype=torch.float16))
    meta = ("s2_scales", "s2_zeros")
    for li, L in enumerate(out["layers"]):
        assert torch.equal(L["ln1"], torch.ones(hid, dtype=torch.float16))      # norms stay ones, as in the reference
        for name in ("qkv", "o"):                                                # attention: what load_llama_w4a8 gives
            assert set(L[name]) == set(llama_like["layers"][li][name])
            assert all(torch.equal(L[name][t], llama_like["layers"][li][name][t]) for t in L[name])
        assert L["gate"].dtype == torch.float16 and torch.equal(L["gate"], state[f"model.layers.{li}.block_sparse_moe.gate.weight"].half())
        gu, dn = L["gate_up"], L["down"]
        assert tuple(gu["qweight"].shape) == (E, 2 * I, hid // 2) and tuple(dn["qweight"].shape) == (E, hid, I // 2)
        assert set(gu) == set(src[li, 0, "w1"]) and set(dn) == set(src[li, 0, "w2"])
        for e in range(E):
            w1, w3, w2 = (src[li, e, n] for n in ("w1", "w3", "w2"))
            for t in gu:
                if t in meta:                                                    # [K/128, N]: the channels are columns
                    assert torch.equal(gu[t][e][:, :I], w1[t]) and torch.equal(gu[t][e][:, I:], w3[t]), (li, e, t)
                else:                                                            # rows 0 .. I-1 = w1 (gate), I .. 2I-1 = w3 (up)
                    assert torch.equal(gu[t][e][:I], w1[t]) and torch.equal(gu[t][e][I:], w3[t]), (li, e, t)
            assert all(torch.equal(dn[t][e], w2[t]) for t in dn), (li, e)
    with pytest.raises(KeyError):
        loader.load_mixtral_w4a8({k: v for k, v in state.items() if "experts.2.w3.qweight" not in k}, CFG, group_size=group_size)
    with pytest.raises(KeyError):
        loader.load_mixtral_w4a8({k: v for k, v in state.items() if "layers.1.block_sparse_moe.gate" not in k}, CFG, group_size=group_size)
