"""Shared-prefix append attention without a GPU: argument validation of the new C entry and of the Python functions (nothing touches
a device), the pure planner and its Python mirror, `shared_prefix_groups`, and a numpy restatement of the two row mappings and the
merge the kernels of qserve_amd/csrc/append_shared.hip implement, on the float64 scores of the oracle composition."""
import ctypes as C

import numpy as np
import pytest
import torch

import _shared_cases as SC
from _append_cases import compose, expected, rotate_rows
from oracle import kvattn

BASE = 1e4
HEADS = ((32, 8), (8, 2), (4, 4), (8, 1), (7, 1), (16, 8), (64, 8))
WS_CAP = 32 << 20
REC_BLOCK = 32 * 130 * 4       # one wave's record block: 32 rows of fp32 O[128], m, l


def test_shared_entry_validates_before_any_device_call(built_lib):
    from qserve_amd._lib import lib

    def call(qkv=16, out=32, cu=1, past=1, kvp=1, go=1, pl=1, sg=1, T=4, B=2, NG=1, msq=4, mgt=4, mb=2, H=8, Hkv=2, dh=128, qs=12 * 128,
             os_=8 * 128, tpb=64, spt=2 * 64, int4=1, zeros=1, mp=64, ms=64, P=1, S=1):
        return lib.qs_append_attention_shared(qkv, out, cu, past, kvp, go, pl, sg, T, B, NG, msq, mgt, mb, H, Hkv, dh, qs, os_, tpb, spt, int4,
                                              zeros, mp, ms, P, S, None)

    for null in ("qkv", "out", "cu", "past", "kvp"):
        assert call(**{null: 0}) == -1 and b"null" in lib.qs_last_error()
    for null in ("go", "pl", "sg"):
        assert call(**{null: 0}) == -1 and b"null group array" in lib.qs_last_error()
    assert call(dh=64, qs=12 * 64, os_=8 * 64) == -2                     # head_dim 64: never instantiated
    assert call(tpb=32) == -2
    assert call(zeros=0) == -2
    assert call(H=8, Hkv=3) == -1 and b"head counts" in lib.qs_last_error()
    assert call(H=18, Hkv=2, qs=22 * 128, os_=18 * 128) == -2            # 9 query heads per KV head
    assert call(spt=2 * 128) == -1                                       # KV4 pages hold 64 bytes per token and head
    assert call(qs=12 * 128 + 4) == -1 and call(qkv=8) == -1             # 16-byte alignment of rows / of the buffer
    assert call(mb=0) == -1
    assert call(NG=0) == -1 and b"num_groups" in lib.qs_last_error()
    assert call(NG=3) == -1 and b"num_groups" in lib.qs_last_error()     # more groups than sequences
    assert call(NG=-1) == -1 and call(mgt=-1) == -1 and call(msq=-1) == -1 and call(T=-1) == -1 and call(B=-1) == -1
    assert call(P=-2) == -1 and b"num_prefix_splits" in lib.qs_last_error()
    assert call(S=-1) == -1 and b"num_suffix_splits" in lib.qs_last_error()
    assert call(P=-2, mp=-1, ms=-1) == -1                                # (negative hints are legal, such counts are not)
    assert call(T=0) == 0 and call(B=0, NG=0) == 0 and call(msq=0) == 0 and call(mgt=0) == 0      # nothing to do: no launch
    assert call(T=0, P=-1, S=0, mp=-1, ms=-1) == 0


def _cpu_args(H=8, Hkv=2):
    qkv = torch.zeros((4, (H + 2 * Hkv) * 128), dtype=torch.float16)     # CPU tensors: every call must fail in the checks
    cu = torch.tensor([0, 2, 4], dtype=torch.int32)
    past = torch.zeros((2,), dtype=torch.int32)
    kvp = torch.zeros((2, 2, 2), dtype=torch.int64)
    return qkv, cu, past, kvp


def test_python_wrappers_raise_before_the_library_is_touched(built_lib):
    from qserve_amd import append as A
    H, Hkv = 8, 2
    qkv, cu, past, kvp = _cpu_args(H, Hkv)
    groups = A.shared_prefix_groups([2], [64])
    with pytest.raises(RuntimeError, match="CUDA"):
        A.append_shared(qkv, cu, past, kvp, H, Hkv, Hkv * 64, BASE, True, groups, max_prefix=64)
    with pytest.raises(RuntimeError, match="CUDA"):
        A.append_attention_shared(qkv, cu, past, kvp, H, Hkv, Hkv * 64, True, groups, num_prefix_splits=2)
    with pytest.raises(RuntimeError, match="scalar type"):
        A.append_attention_shared(qkv.float(), cu, past, kvp, H, Hkv, Hkv * 64, True, groups)
    with pytest.raises(TypeError):
        A.append_attention_shared(None, cu, past, kvp, H, Hkv, Hkv * 64, True, groups)


def test_python_wrapper_checks_shapes_and_counts(built_lib, monkeypatch):
    """The checks behind the dtype / device test, reached with the device test switched off; the library is replaced by a stub that
    fails the test when it is called."""
    from qserve_amd import append as A
    from qserve_amd.backend import _util

    class _NoLib:
        def __getattr__(self, name):
            raise AssertionError(f"the library was called ({name})")

    monkeypatch.setattr(_util, "on_device", lambda t: True)
    monkeypatch.setattr(A, "lib", _NoLib())
    H, Hkv = 8, 2
    qkv, cu, past, kvp = _cpu_args(H, Hkv)
    groups = A.shared_prefix_groups([2], [64])
    call = lambda g=groups, **kw: A.append_attention_shared(qkv, cu, past, kvp, H, Hkv, Hkv * 64, True, g, **kw)      # noqa: E731
    with pytest.raises(RuntimeError, match="triple"):
        call(None)
    with pytest.raises(RuntimeError, match="scalar type"):
        call(tuple(g.long() for g in groups))
    with pytest.raises(RuntimeError, match=r"group_offsets must be \[groups \+ 1\]"):
        call(A.shared_prefix_groups([1, 1, 1], [0, 0, 0]))               # three groups, two sequences
    with pytest.raises(RuntimeError, match=r"group_offsets must be \[groups \+ 1\]"):
        call((groups[0][:1], groups[1], groups[2]))
    with pytest.raises(RuntimeError, match="seq_group"):
        call((groups[0], groups[1], groups[2][:1]))
    with pytest.raises(RuntimeError, match="num_prefix_splits"):
        call(num_prefix_splits=0)
    with pytest.raises(RuntimeError, match="num_prefix_splits"):
        call(num_prefix_splits=-2)
    with pytest.raises(RuntimeError, match="num_suffix_splits"):
        call(num_suffix_splits=0)
    with pytest.raises(RuntimeError, match="max_group_tokens"):
        call(max_group_tokens=-1)
    with pytest.raises(RuntimeError, match="out must be"):
        call(out=torch.zeros((4, H, 64), dtype=torch.float16))


def test_shared_prefix_groups():
    from qserve_amd.append import shared_prefix_groups
    offs, pref, sg = shared_prefix_groups([5, 1, 3], [192, 0, 64], batch=9)
    assert all(t.dtype == torch.int32 and t.device.type == "cpu" for t in (offs, pref, sg))
    assert offs.tolist() == [0, 5, 6, 9] and pref.tolist() == [192, 0, 64] and sg.tolist() == [0] * 5 + [1] + [2] * 3
    offs, pref, sg = shared_prefix_groups(np.array([2]), torch.tensor([0]))
    assert offs.tolist() == [0, 2] and pref.tolist() == [0] and sg.tolist() == [0, 0]
    lay = SC.layout(SC.SIZES, SC.PREFIXES, SC.EXTRAS, SC.NS)             # the test builders agree with the product helper
    offs, pref, sg = shared_prefix_groups(SC.SIZES, SC.PREFIXES)
    assert offs.tolist() == lay["group_offsets"].tolist() and sg.tolist() == lay["seq_group"].tolist()
    for sizes, prefixes, kw, msg in (([], [], {}, "at least one"), ([2, 1], [64], {}, "one each per group"), ([2, 0], [64, 64], {}, "at least one sequence"),
                                     ([2, -1], [64, 64], {}, "at least one sequence"), ([2, 2], [64, 0], dict(batch=5), "sum to 4"),
                                     ([2], [-64], {}, "multiple of 64"), ([2], [100], {}, "multiple of 64"), ([2, 1], [64, 63], {}, "multiple of 64")):
        with pytest.raises(RuntimeError, match=msg):
            shared_prefix_groups(sizes, prefixes, **kw)


def test_shared_plan_is_pure_and_mirrored(built_lib):
    from qserve_amd._lib import lib
    from qserve_amd.plan import append_attention_plan, append_attention_split_plan, append_shared_plan
    buf = (C.c_int * 8)()
    hints = (0, 63, 64, 128, 1024, 8192, 131072)
    for int4 in (1, 0):
        for batch, groups in ((0, 0), (1, 1), (4, 1), (4, 2), (4, 4), (64, 1), (64, 8), (64, 64)):
            for n in (0, 1, 4, 33, 512):
                for H, Hkv in HEADS:
                    mgt = n * (batch // max(groups, 1))                  # equal groups of full sequences
                    base3 = append_attention_plan(batch, n, H, Hkv)
                    for ms in (0, 64, 1024, 8192):
                        prev = 0
                        for mp in hints:
                            assert lib.qs_append_shared_plan(batch, n, groups, mgt, mp, ms, H, Hkv, int4, C.cast(buf, C.c_void_p)) == 0
                            got = append_shared_plan(batch, n, groups, mgt, mp, ms, H, Hkv, bool(int4))
                            assert got == dict(tile_tokens=buf[0], q_tiles=buf[1], waves=buf[2], suffix_splits=buf[3], group_q_tiles=buf[4],
                                               prefix_splits=buf[5], rec_waves_suffix=buf[6] & 0xFF, rec_waves_prefix=buf[6] >> 8,
                                               workspace_bytes=buf[7] * 1024)
                            assert {k: got[k] for k in base3} == base3       # the first fields are qs_append_attention_plan's
                            if batch == 0 or n == 0:
                                assert list(buf) == [0] * 8                  # empty launch
                                continue
                            P, S, tq, G = got["prefix_splits"], got["suffix_splits"], got["tile_tokens"], H // Hkv
                            assert got["group_q_tiles"] == -(-mgt // tq)
                            assert got["workspace_bytes"] <= WS_CAP and 0 <= P <= 64 and 1 <= S <= 64
                            if groups == batch or mp < 64:
                                assert P == 0
                            if P == 0:                                   # "do not share": the split entry's launch over the whole past
                                sp = append_attention_split_plan(batch, n, mp + ms, H, Hkv, bool(int4))
                                assert S == sp["splits"] and got["workspace_bytes"] == sp["workspace_bytes"]
                                assert (got["rec_waves_suffix"], got["rec_waves_prefix"]) == (4, 0)
                                continue
                            assert P <= max(mp // 64, 1) and S <= max(-(-ms // 64), 1)
                            rws, rwp = got["rec_waves_suffix"], got["rec_waves_prefix"]
                            assert rws == min(4, -(-min(tq, n) * G // 32)) and rwp == min(4, -(-min(tq, mgt) * G // 32))
                            need = (P * groups * got["group_q_tiles"] * rwp + S * batch * got["q_tiles"] * rws) * Hkv * REC_BLOCK
                            assert got["workspace_bytes"] - 1024 < need <= got["workspace_bytes"]
                            assert P >= prev or need + REC_BLOCK * Hkv * groups * got["group_q_tiles"] * rwp > WS_CAP, \
                                "prefix splits must not decrease with max_prefix, up to the workspace cut"
                            prev = P
    # S is monotone in the suffix hint at a fixed prefix hint
    for batch, groups, n in ((2, 1, 4), (8, 2, 8), (64, 1, 4)):
        prev = 0
        for ms in (0, 64, 512, 1024, 4096, 8192, 65536):
            s = append_shared_plan(batch, n, groups, n * batch // groups, 1024, ms, 32, 8)
            assert s["prefix_splits"] >= 1 and s["suffix_splits"] >= prev
            prev = s["suffix_splits"]
    # the shapes the feature exists for: one set of suffix records fits although 64 x 8 x 4 blocks of the split entry would not
    p = append_shared_plan(64, 4, 1, 256, 1024, 64, 32, 8)
    assert p["prefix_splits"] >= 1 and p["rec_waves_suffix"] == 1 and p["rec_waves_prefix"] == 4 and p["workspace_bytes"] <= WS_CAP
    assert 64 * 8 * 4 * REC_BLOCK > WS_CAP
    assert append_shared_plan(16, 8, 1, 128, 8192, 512, 32, 8)["prefix_splits"] > 1
    # error codes
    assert lib.qs_append_shared_plan(2, 4, 1, 8, 64, 64, 8, 3, 1, C.cast(buf, C.c_void_p)) == -1 and list(buf) == [0] * 8
    assert lib.qs_append_shared_plan(2, 4, 1, 8, 64, 64, 18, 2, 1, C.cast(buf, C.c_void_p)) == -2
    assert lib.qs_append_shared_plan(2, 4, 1, 8, 64, 64, 8, 2, 1, None) == -1
    for bad in (dict(mp=-1), dict(ms=-1), dict(batch=-1), dict(n=-1), dict(groups=0), dict(groups=3), dict(mgt=-1)):
        a = dict(batch=2, n=4, groups=1, mgt=8, mp=64, ms=64)
        a.update(bad)
        assert lib.qs_append_shared_plan(a["batch"], a["n"], a["groups"], a["mgt"], a["mp"], a["ms"], 8, 2, 1, C.cast(buf, C.c_void_p)) == -1, bad


# ---- the two row mappings and the merge, restated ----------------------------------------------------------------------------------
def _partial(S, V):
    """One range's record for one row, log2 domain (tests/test_append_split_cpu.py): (O un-normalised [128], m, l); no visible key:
    (0, -inf, 0)."""
    if S.size == 0 or not np.isfinite(S).any():
        return np.zeros(128), -np.inf, 0.0
    m = S.max()
    p = np.exp2(S - m)
    return p @ V, m, p.sum()


def _merge(recs):
    """M = max m; out = sum 2^(m - M) O / sum 2^(m - M) l; weight 0 for m = -inf; a row without any key is exactly 0."""
    M = max([m for _, m, _ in recs], default=-np.inf)
    num, den = np.zeros(128), 0.0
    for O, m, l in recs:
        if m == -np.inf:
            continue
        w = np.exp2(m - M)
        num += w * O
        den += w * l
    return num / den if den > 0 else np.zeros(128)


@pytest.mark.parametrize("int4", [True, False], ids=["kv4", "kv8"])
@pytest.mark.parametrize("P,S", [(1, 1), (2, 1), (3, 2), (5, 3)])
@pytest.mark.parametrize("H,Hkv", [(8, 2), (7, 1), (4, 4), (16, 8)])
def test_group_and_sequence_mappings_merge_to_the_oracle_composition(H, Hkv, P, S, int4):
    """One group of five sequences with n = 7, 0, 13, 1, 20 behind a 192-token prefix (pasts 192 + {0, 1, 63, 64, 130}).
    The prefix role's records are written under the GROUP mapping (the group's 41 tokens as one sequence: tile gi / tq, row
    (gi % tq) * G + g, wave row / 32, lane row % 32) from the FIRST member's keys, the suffix role's under the sequence mapping; the
    merge side looks both up again and joins them, prefix records first.  Reference: the float64 softmax over the oracle
    composition's keys, to 1e-9 - `expected` itself is that value rounded to float32, so it is met to float32 rounding (1e-6, the
    bar of tests/test_append_split_cpu.py), not to 1e-9."""
    G, tq = H // Hkv, 128 // (H // Hkv)
    sizes, prefixes, extras, ns = (5,), (192,), SC.EXTRAS[:5], SC.NS[:5]
    lay = SC.layout(sizes, prefixes, extras, ns)
    r = np.random.default_rng(7 * H + Hkv + P)
    own, tables, nblocks, mb = SC.tables_for(r, lay, ns)
    pasts, cu_q, B, W = lay["pasts"], lay["cu_q"], len(ns), (H + 2 * Hkv) * 128
    pool = kvattn.PagePool(nblocks, Hkv, 128, int4, fill=0xFF)
    ctx = r.standard_normal((int(pasts.sum()), W)).astype(np.float16)
    cu_ctx = np.concatenate([[0], np.cumsum(pasts)]).astype(np.int32)
    kvattn.prefill_update_kv_cache(ctx, pasts, kvattn.compute_padding_offsets(cu_ctx, int(pasts.max()), len(ctx)), own, pool, H, Hkv,
                                   int(pasts.max()), BASE)
    rot = rotate_rows(r.standard_normal((int(cu_q[-1]), W)).astype(np.float16), cu_q, pasts, H, Hkv, BASE)
    ref32 = expected(rot, cu_q, pasts, tables, pool, H, Hkv)
    q, K, V, cu_k = compose(rot, cu_q, pasts, tables, pool, H, Hkv)
    q, K, V = q.astype(np.float64), K.astype(np.float64), V.astype(np.float64)
    c = np.log2(np.e) / np.sqrt(128)
    prefix, first = prefixes[0], 0
    # ---- the prefix role: group tiles x KV heads x prefix splits, rows of the group's tokens, keys of the FIRST member
    prec, n_group, q0 = {}, int(lay["group_tokens"][0]), int(cu_q[first])
    for tile in range(-(-n_group // tq)):
        for hkv in range(Hkv):
            for s in range(P):
                p0, npg = SC.split_range(prefix, s, P)
                if npg == 0:
                    continue                                             # EMPTY: no record
                keys = int(cu_k[first]) + np.arange(p0 * 64, (p0 + npg) * 64)
                for row in range(tq * G):
                    tok = tile * tq + row // G
                    if tok < n_group:
                        prec[(tile, hkv, s, row // 32, row % 32)] = _partial(K[keys, hkv] @ q[q0 + tok, hkv * G + row % G] * c, V[keys, hkv])
    # ---- the suffix role: sequence tiles x KV heads x suffix splits over the pages from prefix / 64 on, the last with the new tokens
    srec = {}
    for b in range(B):
        n, past_sfx, k0 = int(ns[b]), int(pasts[b]) - prefix, int(cu_k[b])
        for qt in range(-(-n // tq)):
            for hkv in range(Hkv):
                for s in range(S):
                    p0, npg = SC.split_range(past_sfx, s, S)
                    if npg == 0 and s != S - 1:
                        continue
                    cached = np.arange(prefix + p0 * 64, min(prefix + (p0 + npg) * 64, int(pasts[b])))
                    for row in range(tq * G):
                        i = qt * tq + row // G
                        if i < n:
                            keys = k0 + np.concatenate([cached, np.arange(pasts[b], pasts[b] + i + 1) if s == S - 1 else []]).astype(int)
                            srec[(b, qt, hkv, s, row // 32, row % 32)] = _partial(K[keys, hkv] @ q[int(cu_q[b]) + i, hkv * G + row % G] * c,
                                                                                  V[keys, hkv])
    # ---- the merge: sequence mapping for the output row and the suffix records, group mapping for the prefix records
    got = np.zeros(ref32.shape, np.float64)
    direct = np.zeros(ref32.shape, np.float64)
    empty_p = 0
    for b in range(B):
        past_sfx = int(pasts[b]) - prefix
        for i in range(int(ns[b])):
            for h in range(H):
                hkv, g = h // G, h % G
                gi = int(cu_q[b]) - q0 + i
                grow, row = (gi % tq) * G + g, (i % tq) * G + g
                recs = []
                for s in range(P):
                    if SC.split_range(prefix, s, P)[1] > 0:
                        recs.append(prec[(gi // tq, hkv, s, grow // 32, grow % 32)])
                    else:
                        empty_p += 1
                for s in range(S):
                    if SC.split_range(past_sfx, s, S)[1] > 0 or s == S - 1:
                        recs.append(srec[(b, i // tq, hkv, s, row // 32, row % 32)])
                got[int(cu_q[b]) + i, h] = _merge(recs)
                keys = int(cu_k[b]) + np.arange(int(pasts[b]) + i + 1)
                direct[int(cu_q[b]) + i, h] = _merge([_partial(K[keys, hkv] @ q[int(cu_q[b]) + i, h] * c, V[keys, hkv])])
    assert (P <= 3) == (empty_p == 0), "P = 5 over 3 pages must hold empty prefix splits"
    assert len({k[0] for k in prec}) >= (2 if G >= 4 else 1) and len({k[3] for k in prec}) >= 2      # tile and wave boundaries crossed
    assert np.isfinite(got).all()
    assert np.abs(got - direct).max() <= 1e-9
    assert np.abs(direct - ref32).max() <= 1e-6 and np.abs(got - ref32).max() <= 1e-6
