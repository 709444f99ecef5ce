"""LoRA rows on the CPU: the float64 oracle of tests/_lora_cases.py against an independent torch index_select + bmm restatement,
`lora.LoraTable.load` on PEFT-named tensors against a qkv / gate_up split written out by hand, and every argument rule of
`qs_lora_rows`, which answers before any device call."""
import numpy as np
import pytest
import torch

import _lora_cases as K

CFG = dict(name="lora-test", hidden=256, heads=4, kv_heads=2, inter=512, layers=2, vocab=512, rope_theta=1e4, eps=1e-5)


@pytest.fixture(scope="module")
def lora(built_lib):
    from qserve_amd import lora
    return lora


# ---- the oracle ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["one_row", "one_seq_r64", "step_64", "tree_12_r8", "three_j_groups"])
def test_oracle_against_index_select_and_bmm(name):
    """Gather every row's adapter with index_select, one bmm per stage and segment, in float64; rows of an id out of range keep `out`."""
    c = K.make_case(name)
    out, x = K.views(c)
    y, M, active = K.case_oracle(c)
    T, r, slots = c["T"], c["r"], c["slots"]
    row_a = torch.from_numpy(np.repeat(c["seq_adapter"], c["rows_per_seq"]).astype(np.int64))
    ok = (row_a >= 0) & (row_a < slots)
    assert ok.numpy().tolist() == active.tolist()
    idx = row_a.clamp(0, slots - 1)
    A = torch.index_select(torch.from_numpy(c["A"]).double(), 0, idx)                   # [T, nseg r, K]
    B = torch.index_select(torch.from_numpy(c["B"]).double(), 0, idx)                   # [T, N, r]
    sc = torch.index_select(torch.from_numpy(c["scaling"]).double(), 0, idx)
    t = torch.bmm(A, torch.from_numpy(x).double().unsqueeze(2)).squeeze(2) * torch.from_numpy(c["x_scale"]).double().unsqueeze(1)
    want = torch.from_numpy(out).double().clone()
    n0 = 0
    for g, n1 in enumerate(c["seg_ends"]):
        d = torch.bmm(B[:, n0:n1], t[:, g * r:(g + 1) * r].unsqueeze(2)).squeeze(2) * sc.unsqueeze(1)
        want[:, n0:n1] += torch.where(ok.unsqueeze(1), d, torch.zeros_like(d))
        n0 = n1
    assert np.allclose(y, want.numpy(), rtol=1e-12, atol=1e-12)
    assert np.array_equal(y[~active], out[~active].astype(np.float64)) and (M[~active] == 0).all()
    assert (np.abs(y - out)[active] > 0).mean() > 0.99 and (M[active] > 0).all(), "the adapters hardly change the rows"
    assert (np.abs(y - out.astype(np.float64)) <= M * (1 + 1e-9)).all(), "M does not bound the delta"


def test_the_cases_cover_what_they_say():
    seen_r, seen_T, seen_rps = set(), set(), set()
    for name, (T, rps, Kk, N, ends, r, slots, ids) in K.SHAPES.items():
        c = K.make_case(name)
        assert T % rps == 0 and Kk % 128 == 0 and ends[-1] == N and all(e % 64 == 0 for e in ends)
        assert c["out_store"].shape == (T + 2, N + 8) and c["x_store"].shape == (T + 2, Kk + 16)
        seen_r.add(r), seen_T.add(T), seen_rps.add(rps)
    assert seen_r == {8, 16, 32, 64} and seen_T >= {1, 3, 64, 130} and seen_rps == {1, 3, 5, 12, 65}
    for name in ("step_64", "many_short_seqs"):
        ids, slots = K.make_case(name)["seq_adapter"].tolist(), K.SHAPES[name][6]
        assert {-1, slots, -7} <= set(ids) and len({i for i in ids if 0 <= i < slots}) >= 2, name


# ---- LoraTable ----------------------------------------------------------------------------------------------------------------------
def test_load_places_every_module_in_its_segment(lora):
    """q / k / v and gate / up against slices written out by hand for hidden 256, 4 heads, 2 KV heads (128 wide), inter 512: the fused
    qkv has rows 0 .. 511 | 512 .. 767 | 768 .. 1023, gate_up 0 .. 511 | 512 .. 1023; segment g owns rows g * rank .. of A."""
    rank, r1 = 16, 8
    t = lora.LoraTable(CFG, slots=3, rank=rank, device="cpu")
    assert t.shapes == dict(qkv=(256, 1024, (512, 768, 1024)), o=(512, 256, (256,)), gate_up=(256, 1024, (512, 1024)), down=(512, 256, (256,)))
    assert all((A == 0).all() and (B == 0).all() for layer in t.layers for A, B in layer.values()) and (t.scaling == 0).all()
    ad = K.peft_adapter(CFG, r1, seed=3, skip={(1, "k"), (0, "down")})
    ad["base_model.model.model.norm.weight"] = torch.ones(256)                        # (a key of another form: ignored)
    t.load(1, ad, alpha=32)
    assert t.scaling.tolist() == [0.0, 4.0, 0.0]

    def w(li, block, mod, ab):
        return ad[f"{K.PREFIX}{li}.{block}.{mod}_proj.lora_{ab}.weight"]

    for li in range(2):
        A, B = t.layers[li]["qkv"]
        assert tuple(A.shape) == (3, 48, 256) and tuple(B.shape) == (3, 1024, 16)
        assert torch.equal(A[1, 0:8], w(li, "self_attn", "q", "A")) and torch.equal(B[1, 0:512, :8], w(li, "self_attn", "q", "B"))
        assert torch.equal(A[1, 32:40], w(li, "self_attn", "v", "A")) and torch.equal(B[1, 768:1024, :8], w(li, "self_attn", "v", "B"))
        if li == 0:
            assert torch.equal(A[1, 16:24], w(0, "self_attn", "k", "A")) and torch.equal(B[1, 512:768, :8], w(0, "self_attn", "k", "B"))
        else:                                                                         # a missing module stays zero
            assert (A[1, 16:32] == 0).all() and (B[1, 512:768] == 0).all()
        assert (A[1, 8:16] == 0).all() and (A[1, 24:32] == 0).all() and (A[1, 40:48] == 0).all() and (B[1, :, 8:] == 0).all()   # rank padding
        A, B = t.layers[li]["gate_up"]
        assert torch.equal(A[1, 0:8], w(li, "mlp", "gate", "A")) and torch.equal(B[1, 0:512, :8], w(li, "mlp", "gate", "B"))
        assert torch.equal(A[1, 16:24], w(li, "mlp", "up", "A")) and torch.equal(B[1, 512:1024, :8], w(li, "mlp", "up", "B"))
        A, B = t.layers[li]["o"]
        assert torch.equal(A[1, 0:8], w(li, "self_attn", "o", "A")) and torch.equal(B[1, :, :8], w(li, "self_attn", "o", "B"))
        A, B = t.layers[li]["down"]
        if li == 0:
            assert (A[1] == 0).all() and (B[1] == 0).all()
        else:
            assert torch.equal(A[1, 0:8], w(1, "mlp", "down", "A")) and torch.equal(B[1, :, :8], w(1, "mlp", "down", "B"))
        for A, B in t.layers[li].values():                                            # the other slots were not touched
            assert (A[0] == 0).all() and (A[2] == 0).all() and (B[0] == 0).all() and (B[2] == 0).all()
    # a second load of the slot replaces the first; unload zeroes it
    t.load(1, K.peft_adapter(CFG, 16, seed=4, skip={(li, m) for li in range(2) for _, m in K.MODULES if m != "o"}), alpha=8)
    assert t.scaling[1] == 0.5 and (t.layers[0]["qkv"][0] == 0).all() and (t.layers[0]["o"][0][1] != 0).any()
    t.unload(1)
    assert all((A == 0).all() and (B == 0).all() for layer in t.layers for A, B in layer.values()) and (t.scaling == 0).all()


def test_zero_padding_a_rank_is_exact():
    """The oracle on an adapter of rank 8 and on the same adapter padded to 16 with zeros: the same float64 values."""
    c = K.make_case("tree_12_r8")
    y8, _, _ = K.case_oracle(c)
    r, nseg = 8, 3
    A16 = np.zeros((c["slots"], nseg * 16, c["K"]), dtype=np.float16)
    B16 = np.zeros((c["slots"], c["N"], 16), dtype=np.float16)
    for g in range(nseg):
        A16[:, g * 16:g * 16 + r] = c["A"][:, g * r:(g + 1) * r]
    B16[:, :, :r] = c["B"]
    out, x = K.views(c)
    y16, _, _ = K.oracle(out, x, c["x_scale"], A16, B16, c["scaling"], c["seq_adapter"], c["rows_per_seq"], c["seg_ends"])
    assert np.array_equal(y8, y16)


def test_load_refuses_what_it_cannot_place(lora):
    t = lora.LoraTable(CFG, slots=2, rank=16, device="cpu")
    good = K.peft_adapter(CFG, 8, seed=1)
    t.load(0, good, alpha=16)
    before = [(A.clone(), B.clone()) for layer in t.layers for A, B in layer.values()]
    q_a, q_b = f"{K.PREFIX}0.self_attn.q_proj.lora_A.weight", f"{K.PREFIX}0.self_attn.q_proj.lora_B.weight"
    with pytest.raises(ValueError, match="rank 32, the table holds rank <= 16"):
        t.load(0, K.peft_adapter(CFG, 32, seed=2), alpha=16)
    with pytest.raises(ValueError, match=r"must be \[r, 256\] / \[512, r\]"):
        t.load(0, {**good, q_a: torch.zeros((8, 128), dtype=torch.float16)}, alpha=16)
    with pytest.raises(ValueError, match=r"must be \[r, 256\] / \[512, r\]"):
        t.load(0, {**good, q_b: torch.zeros((256, 8), dtype=torch.float16)}, alpha=16)
    with pytest.raises(ValueError, match="one rank per adapter"):
        t.load(0, {**good, q_a: torch.zeros((4, 256), dtype=torch.float16), q_b: torch.zeros((512, 4), dtype=torch.float16)}, alpha=16)
    with pytest.raises(ValueError, match="lora_A only"):
        t.load(0, {k: v for k, v in good.items() if k != q_b}, alpha=16)
    with pytest.raises(ValueError, match="the model has 2 layers"):
        t.load(0, {**good, f"{K.PREFIX}2.mlp.up_proj.lora_A.weight": torch.zeros((8, 256))}, alpha=16)
    with pytest.raises(ValueError, match="no `...layers"):
        t.load(0, {"lm_head.weight": torch.zeros((4, 4))}, alpha=16)
    with pytest.raises(ValueError, match="slot=2"):
        t.load(2, good, alpha=16)
    with pytest.raises(ValueError, match="rank=12"):
        lora.LoraTable(CFG, slots=2, rank=12, device="cpu")
    after = [(A, B) for layer in t.layers for A, B in layer.values()]
    assert all(torch.equal(a0, a1) and torch.equal(b0, b1) for (a0, b0), (a1, b1) in zip(before, after)), "a refused load changed the slot"
    assert t.scaling.tolist() == [2.0, 0.0]


# ---- the argument rules ---------------------------------------------------------------------------------------------------------------
OK = dict(out=256, ostride=1032, x=512, xstride=272, xs=64, A=1024, B=2048, sc=64, ids=64, slots=4, T=36, K=256, N=1024, r=16, rps=12,
          nseg=3, e0=512, e1=768, e2=1024, ws=4096, wsb=1 << 20)


def _call(lib, **kw):
    a = {**OK, **kw}
    return lib.qs_lora_rows(a["out"], a["ostride"], a["x"], a["xstride"], a["xs"], a["A"], a["B"], a["sc"], a["ids"], a["slots"], a["T"],
                            a["K"], a["N"], a["r"], a["rps"], a["nseg"], a["e0"], a["e1"], a["e2"], a["ws"], a["wsb"], None)


def test_library_refuses_bad_arguments_without_a_device(built_lib):
    """QS_EINVAL comes before any device call, so the C ABI itself can be asked on a machine without a GPU: the addresses are never
    dereferenced, and a launch would fail here with another code than -1.  T = 0 with good arguments is QS_OK and launches nothing."""
    from qserve_amd._lib import lib
    assert _call(lib, T=0) == 0
    bad = [dict(out=0), dict(x=0), dict(xs=0), dict(A=0), dict(B=0), dict(sc=0), dict(ids=0), dict(ws=0),
           dict(r=0), dict(r=12), dict(r=128), dict(K=0), dict(K=192, xstride=192), dict(K=(1 << 20) + 128, xstride=(1 << 20) + 128),
           dict(N=0, e2=0), dict(N=1056, e2=1056, ostride=1056), dict(nseg=0), dict(nseg=4),
           dict(e0=500), dict(e0=768, e1=512), dict(e1=768, e0=768), dict(e2=960), dict(nseg=2), dict(nseg=1, e0=512), dict(e0=0),
           dict(slots=0), dict(T=-12), dict(T=(1 << 24) + 12), dict(rps=0), dict(rps=7), dict(rps=-12),
           dict(xstride=128), dict(xstride=264), dict(ostride=1016), dict(ostride=1028),
           dict(out=264), dict(x=520), dict(A=1032), dict(B=2056), dict(ws=4104), dict(xs=65), dict(sc=66), dict(ids=66),
           dict(wsb=36 * 48 * 4 - 1)]
    for kw in bad:
        assert _call(lib, **kw) == -1, kw
        assert lib.qs_last_error().startswith(b"lora_rows:"), (kw, lib.qs_last_error())
    assert lib.qs_lora_rows_workspace(36, 256, 16, 3) == 36 * 48 * 4 and lib.qs_lora_rows_workspace(3, 14336, 16, 2) == 28 * 3 * 32 * 4
    assert lib.qs_lora_rows_workspace(0, 128, 8, 1) == 0
    for args in ((-1, 256, 16, 3), (36, 200, 16, 3), (36, 256, 24, 3), (36, 256, 16, 0), (36, 256, 16, 4)):
        assert lib.qs_lora_rows_workspace(*args) == -1, args
    assert lib.qs_last_error().startswith(b"lora_rows_workspace:")


def test_wrapper_checks_match_the_library(lora):
    """`lora.lora_rows` refuses the same shapes with a message of its own, before it asks for a device; CPU tensors that pass every shape
    rule are refused by the device check, the last one in front of the library."""
    def args(**kw):
        a = dict(out=torch.zeros((36, 1024), dtype=torch.float16), x=torch.zeros((36, 256), dtype=torch.int8),
                 x_scale=torch.zeros(36, dtype=torch.float16), A=torch.zeros((4, 48, 256), dtype=torch.float16),
                 B=torch.zeros((4, 1024, 16), dtype=torch.float16), scaling=torch.zeros(4), seq_adapter=torch.zeros(3, dtype=torch.int32),
                 rows_per_seq=12, seg_ends=(512, 768, 1024))
        a.update(kw)
        return a

    for kw, msg in ((dict(x=torch.zeros((36, 256), dtype=torch.int16)), "expected scalar type torch.int8 for x"),
                    (dict(out=[0]), "out must be a torch.Tensor"),
                    (dict(seg_ends=(512, 700, 1024)), "seg_ends="), (dict(seg_ends=(512, 1024, 768)), "seg_ends="),
                    (dict(seg_ends=(512, 768)), "seg_ends="), (dict(seg_ends=(256, 512, 768, 1024)), "seg_ends="),
                    (dict(B=torch.zeros((4, 1024, 12), dtype=torch.float16)), r"B must be \[slots, N=1024, r\]"),
                    (dict(A=torch.zeros((4, 16, 256), dtype=torch.float16)), r"A must be \[4, 48, K=256\]"),
                    (dict(scaling=torch.zeros(3)), r"scaling \[4\]"),
                    (dict(x=torch.zeros((36, 192), dtype=torch.int8), A=torch.zeros((4, 48, 192), dtype=torch.float16)), "K=192 must be a multiple of 128"),
                    (dict(rows_per_seq=7), "multiple of rows_per_seq=7"), (dict(rows_per_seq=0), "rows_per_seq=0"),
                    (dict(seq_adapter=torch.zeros(36, dtype=torch.int32)), "one id per sequence"),
                    (dict(x_scale=torch.zeros(35, dtype=torch.float16)), "x_scale"),
                    (dict(out=torch.zeros((36, 1028), dtype=torch.float16)[:, :1024]), "row strides of out"),
                    (dict(x=torch.zeros((36, 264), dtype=torch.int8)[:, :256]), "row strides of out")):
        with pytest.raises((RuntimeError, TypeError), match=msg):
            lora.lora_rows(**args(**kw))
    with pytest.raises(RuntimeError, match="out must be on CUDA"):
        lora.lora_rows(**args())
    assert lora.workspace_bytes(36, 256, 16, 3) == 36 * 48 * 4
    with pytest.raises(RuntimeError, match="lora_rows_workspace"):
        lora.workspace_bytes(36, 200, 16, 3)
