"""Split-KV append attention without a GPU: argument validation of the new C entry and of the Python wrappers (nothing touches a
device), the pure split planner and its Python mirror, and the partial-record / merge arithmetic the two kernels implement
(qserve_amd/csrc/append_attention_split.hip), restated in numpy on the float64 scores of the oracle composition."""
import ctypes as C

import numpy as np
import pytest
import torch

from _append_cases import compose, expected, rotate_rows, scattered_tables
from oracle import kvattn

BASE = 1e4
HEADS = ((32, 8), (8, 2), (4, 4), (8, 1), (6, 2), (12, 4), (5, 1), (7, 1), (16, 8), (28, 4), (64, 8))   # test_append_cpu.py's
WS_CAP = 32 << 20
REC_BYTES = 130 * 4        # one row's partial record: fp32 O[128], m, l


def test_split_entry_validates_before_any_device_call(built_lib):
    from qserve_amd._lib import lib

    def call(qkv=16, out=32, cu=1, past=1, kvp=1, T=4, B=1, msq=4, mb=2, H=8, Hkv=2, dh=128, qs=12 * 128, os_=8 * 128, tpb=64,
             spt=2 * 64, int4=1, zeros=1, max_past=128, splits=2):
        return lib.qs_append_attention_split(qkv, out, cu, past, kvp, T, B, msq, mb, H, Hkv, dh, qs, os_, tpb, spt, int4, zeros,
                                             max_past, splits, None)

    for null in ("qkv", "out", "cu", "past", "kvp"):
        assert call(**{null: 0}) == -1 and b"null" in lib.qs_last_error()
    assert call(dh=64, qs=12 * 64, os_=8 * 64) == -2                     # head_dim 64: never instantiated
    assert call(tpb=32) == -2
    assert call(zeros=0) == -2
    assert call(H=8, Hkv=3) == -1 and b"head counts" in lib.qs_last_error()
    assert call(H=18, Hkv=2, qs=22 * 128, os_=18 * 128) == -2            # 9 query heads per KV head
    assert call(spt=2 * 128) == -1                                       # KV4 pages hold 64 bytes per token and head
    assert call(qs=12 * 128 + 4) == -1 and call(qkv=8) == -1             # 16-byte alignment of rows / of the buffer
    assert call(mb=0) == -1
    assert call(splits=-1) == -1 and b"num_splits" in lib.qs_last_error()
    assert call(splits=-1, max_past=-1) == -1                            # (a negative hint is legal, a negative count is not)
    assert call(T=0) == 0 and call(B=0) == 0 and call(msq=0) == 0        # nothing to do: no launch


def test_python_wrappers_raise_before_the_library_is_touched(built_lib):
    from qserve_amd import append as A
    H, Hkv = 8, 2
    qkv = torch.zeros((4, (H + 2 * Hkv) * 128), dtype=torch.float16)     # CPU tensors: every call must fail in the checks
    cu = torch.tensor([0, 4], dtype=torch.int32)
    past = torch.zeros((1,), dtype=torch.int32)
    kvp = torch.zeros((1, 2, 2), dtype=torch.int64)
    with pytest.raises(RuntimeError, match="CUDA"):
        A.append(qkv, cu, past, kvp, H, Hkv, Hkv * 64, BASE, True, max_past=64, num_splits=2)
    with pytest.raises(RuntimeError, match="CUDA"):
        A.append_attention(qkv, cu, past, kvp, H, Hkv, Hkv * 64, True, max_past=64)
    with pytest.raises(RuntimeError, match="scalar type"):
        A.append_attention(qkv.float(), cu, past, kvp, H, Hkv, Hkv * 64, True, num_splits=2)
    with pytest.raises(TypeError):
        A.append_attention(None, cu, past, kvp, H, Hkv, Hkv * 64, True, num_splits=2)


def test_split_plan_is_pure_and_mirrored(built_lib):
    from qserve_amd._lib import lib
    from qserve_amd.plan import append_attention_plan, append_attention_split_plan
    buf = (C.c_int * 5)()
    pasts = (0, 63, 64, 127, 128, 1024, 8192, 32768, 131072)
    for int4 in (1, 0):
        for batch in (0, 1, 4, 64):
            for n in (0, 1, 8, 33, 512):
                for H, Hkv in HEADS:
                    prev = 0
                    for mp in pasts:
                        assert lib.qs_append_attention_split_plan(batch, n, mp, H, Hkv, int4, C.cast(buf, C.c_void_p)) == 0
                        got = append_attention_split_plan(batch, n, mp, H, Hkv, bool(int4))
                        assert got == dict(tile_tokens=buf[0], q_tiles=buf[1], waves=buf[2], splits=buf[3], workspace_bytes=buf[4] * 1024)
                        base3 = append_attention_plan(batch, n, H, Hkv)
                        assert {k: got[k] for k in base3} == base3
                        if batch == 0 or n == 0:
                            assert list(buf) == [0] * 5                  # empty launch
                            continue
                        wgs = batch * Hkv * got["q_tiles"]
                        pages = -(-mp // 64)
                        s = got["splits"]
                        assert s >= 1
                        if wgs >= 512 or mp < 128:
                            assert s == 1
                        assert s <= max(pages, 1) and s <= 64
                        assert got["workspace_bytes"] <= WS_CAP
                        if s > 1:
                            G = H // Hkv
                            valid_rows = min(n, got["tile_tokens"]) * G      # per workgroup, at most
                            assert got["workspace_bytes"] >= s * wgs * valid_rows * REC_BYTES
                        else:
                            assert got["workspace_bytes"] == 0               # the un-split launch has no partial records
                        assert s >= prev, "splits must not decrease with max_past"
                        prev = s
    # the case the feature exists for
    assert append_attention_split_plan(1, 8, 8192, 32, 8)["splits"] > 1
    assert append_attention_split_plan(1, 8, 8192, 32, 8, False)["splits"] > 1
    # the engine tests' shapes (TINY, B = 3, past <= 192, chunk 48): today's launch
    assert append_attention_split_plan(3, 48, 192, 8, 2)["splits"] == 1
    # error codes of the existing plan entry
    assert lib.qs_append_attention_split_plan(1, 4, 128, 8, 3, 1, C.cast(buf, C.c_void_p)) == -1 and list(buf) == [0] * 5
    assert lib.qs_append_attention_split_plan(1, 4, 128, 18, 2, 1, C.cast(buf, C.c_void_p)) == -2
    assert lib.qs_append_attention_split_plan(1, 4, 128, 8, 2, 1, None) == -1
    assert lib.qs_append_attention_split_plan(1, 4, -1, 8, 2, 1, C.cast(buf, C.c_void_p)) == -1
    assert lib.qs_append_attention_split_plan(-1, 4, 128, 8, 2, 1, C.cast(buf, C.c_void_p)) == -1


def _partial(S, V):
    """One range's record for one row, log2 domain: S float64 [keys] (scores in log2 units, -inf = masked), V [keys, 128]
    -> (O un-normalised [128], m, l); a range without a visible key is (0, -inf, 0)."""
    if S.size == 0 or not np.isfinite(S).any():
        return np.zeros(128), -np.inf, 0.0
    m = S.max()
    p = np.exp2(S - m)
    return p @ V, m, p.sum()


def _merge(recs):
    """The merge kernel's formula: M = max m_s; out = sum 2^(m_s - M) O_s / sum 2^(m_s - M) l_s; weight 0 for m_s = -inf; a row
    without any key is exactly 0."""
    M = max(m for _, m, _ in recs)
    num, den = np.zeros(128), 0.0
    for O, m, l in recs:
        if m == -np.inf:
            continue
        w = np.exp2(m - M)
        num += w * O
        den += w * l
    return num / den if den > 0 else np.zeros(128)


@pytest.mark.parametrize("int4", [True, False], ids=["kv4", "kv8"])
@pytest.mark.parametrize("splits", [1, 2, 3, 7, 16])
def test_partial_records_merge_to_the_oracle_composition(splits, int4):
    """Pins the record definition: split s of a sequence covers pages [s pps, min((s + 1) pps, np)) with np = ceil(past / 64),
    pps = ceil(np / splits); the LAST split also holds the new tokens (causal); the other ranges may be empty."""
    H, Hkv, G = 4, 2, 2
    r = np.random.default_rng(40 + splits)
    pasts, ns = [0, 70, 200, 64], [3, 2, 5, 0]
    B, W = len(pasts), (H + 2 * Hkv) * 128
    tables, nblocks = scattered_tables(r, B, 5)
    pool = kvattn.PagePool(nblocks, Hkv, 128, int4, fill=0xFF)
    live = [b for b in range(B) if pasts[b] > 0]
    ctx = r.standard_normal((sum(pasts[b] for b in live), W)).astype(np.float16)
    cu_ctx = np.concatenate([[0], np.cumsum([pasts[b] for b in live])]).astype(np.int32)
    mx = max(pasts)
    kvattn.prefill_update_kv_cache(ctx, np.asarray([pasts[b] for b in live]), kvattn.compute_padding_offsets(cu_ctx, mx, len(ctx)),
                                   tables[live], pool, H, Hkv, mx, BASE)
    cu_q = np.concatenate([[0], np.cumsum(ns)]).astype(np.int32)
    past = np.asarray(pasts, np.int32)
    rot = rotate_rows(r.standard_normal((int(cu_q[-1]), W)).astype(np.float16), cu_q, past, H, Hkv, BASE)
    ref = expected(rot, cu_q, past, tables, pool, H, Hkv)
    q, K, V, cu_k = compose(rot, cu_q, past, tables, pool, H, Hkv)
    got = np.zeros_like(ref, dtype=np.float64)
    empties = 0
    for b in range(B):
        p, n, k0 = pasts[b], ns[b], int(cu_k[b])
        npg = -(-p // 64)
        pps = -(-npg // splits)
        ranges = []
        for s in range(splits):
            a, e = min(s * pps, npg) * 64, min(min((s + 1) * pps, npg) * 64, p)
            ranges.append((a, max(a, e), s == splits - 1))
        assert sum(e - a for a, e, _ in ranges) == p
        empties += sum(1 for a, e, new in ranges if e == a and not new)
        for i in range(n):
            for h in range(H):
                qv = q[int(cu_q[b]) + i, h].astype(np.float64)
                recs = []
                for a, e, new in ranges:
                    idx = list(range(a, e)) + (list(range(p, p + i + 1)) if new else [])
                    Kr, Vr = K[k0 + np.asarray(idx, int), h // G].astype(np.float64), V[k0 + np.asarray(idx, int), h // G].astype(np.float64)
                    recs.append(_partial(Kr @ qv / np.sqrt(128) * np.log2(np.e), Vr))
                got[int(cu_q[b]) + i, h] = _merge(recs)
    assert splits == 1 or empties > 0, "the case must hold empty ranges"
    assert np.isfinite(got).all()
    assert np.abs(got - ref).max() <= 1e-6
