"""Append attention without a GPU: argument validation of the C entries and of the Python wrappers (nothing touches a device),
the pure launch plan, and the pin of the expected-value composition (tests/_append_cases.py) to the existing decode oracle."""
import ctypes as C

import numpy as np
import pytest
import torch

from _append_cases import expected, rotate_rows, scattered_tables
from _helpers import ulp_diff_f16
from oracle import kvattn

BASE = 1e4


def test_attention_entry_validates_before_any_device_call(built_lib):
    from qserve_amd._lib import lib

    def call(qkv=16, out=32, cu=1, past=1, kvp=1, T=4, B=1, msq=4, mb=2, H=8, Hkv=2, dh=128, qs=12 * 128, os_=8 * 128, tpb=64,
             spt=2 * 64, int4=1, zeros=1):
        return lib.qs_append_attention(qkv, out, cu, past, kvp, T, B, msq, mb, H, Hkv, dh, qs, os_, tpb, spt, int4, zeros, None)

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


def test_writer_entry_validates_before_any_device_call(built_lib):
    from qserve_amd._lib import lib

    def call(qkv=16, cu=1, past=1, kvp=1, T=4, B=1, mb=2, H=8, Hkv=2, tpb=64, spt=2 * 64, rot=128, int4=1, zeros=1):
        return lib.qs_append_rope_update_kv_cache(qkv, cu, past, kvp, T, B, mb, H, Hkv, tpb, spt, rot, 1e4, int4, zeros, None)

    for null in ("qkv", "cu", "past", "kvp"):
        assert call(**{null: 0}) == -1 and b"null" in lib.qs_last_error()
    assert call(rot=64) == -2 and call(tpb=32) == -2 and call(zeros=0) == -2
    assert call(spt=100) == -1 and call(mb=0) == -1 and call(H=0) == -1
    assert call(T=0) == 0                                                # nothing to do: no launch


def test_python_wrappers_raise_before_the_library_is_touched(built_lib):
    from qserve_amd import append as A
    H, Hkv = 8, 2
    qkv = torch.zeros((4, (H + 2 * Hkv) * 128), dtype=torch.float16)     # CPU tensors: every call must fail in the checks
    cu = torch.tensor([0, 4], dtype=torch.int32)
    past = torch.zeros((1,), dtype=torch.int32)
    kvp = torch.zeros((1, 2, 2), dtype=torch.int64)
    with pytest.raises(RuntimeError, match="CUDA"):
        A.append(qkv, cu, past, kvp, H, Hkv, Hkv * 64, BASE, True)
    with pytest.raises(RuntimeError, match="scalar type"):
        A.append_attention(qkv.float(), cu, past, kvp, H, Hkv, Hkv * 64, True)
    with pytest.raises(RuntimeError, match="scalar type"):
        A.append_rope_update_kv_cache(qkv.to(torch.bfloat16), cu, past, kvp, H, Hkv, Hkv * 64, BASE, True)
    with pytest.raises(TypeError):
        A.append_attention(None, cu, past, kvp, H, Hkv, Hkv * 64, True)


@pytest.mark.gpu
def test_python_wrappers_check_shapes_and_strides(gpu):
    """(device tensors: the shape / stride checks sit behind the device check; still no launch)"""
    from qserve_amd import append as A
    H, Hkv, d = 8, 2, gpu
    qkv = torch.zeros((4, (H + 2 * Hkv) * 128), dtype=torch.float16, device=d)
    cu = torch.tensor([0, 4], dtype=torch.int32, device=d)
    past = torch.zeros((1,), dtype=torch.int32, device=d)
    kvp = torch.zeros((1, 2, 2), dtype=torch.int64, device=d)
    with pytest.raises(RuntimeError, match="contiguous"):
        A.append_attention(qkv[:, ::2], cu, past, kvp, H, Hkv, Hkv * 64, True)
    with pytest.raises(RuntimeError, match="head counts"):
        A.append_attention(qkv, cu, past, kvp, H, 3, 3 * 64, True)
    with pytest.raises(RuntimeError, match="size_per_token"):
        A.append_attention(qkv, cu, past, kvp, H, Hkv, Hkv * 128, True)
    with pytest.raises(RuntimeError, match="kv_pointers"):
        A.append_attention(qkv, cu, past, kvp[:, 0], H, Hkv, Hkv * 64, True)
    with pytest.raises(RuntimeError, match="out must be"):
        A.append_attention(qkv, cu, past, kvp, H, Hkv, Hkv * 64, True, out=torch.zeros((4, H, 64), dtype=torch.float16, device=d))


def test_plan_is_pure_and_mirrored(built_lib):
    from qserve_amd._lib import lib
    from qserve_amd.plan import append_attention_plan
    buf = (C.c_int * 3)()
    for batch in (0, 1, 4, 64):
        for n in (0, 1, 4, 31, 32, 33, 128, 129, 512, 8192):
            for H, Hkv in ((32, 8), (8, 2), (4, 4), (8, 1), (6, 2), (12, 4), (5, 1), (7, 1), (16, 8), (28, 4), (64, 8)):
                assert lib.qs_append_attention_plan(batch, n, H, Hkv, C.cast(buf, C.c_void_p)) == 0
                got = dict(tile_tokens=buf[0], q_tiles=buf[1], waves=buf[2])
                assert got == append_attention_plan(batch, n, H, Hkv)
                if batch == 0 or n == 0:
                    assert list(buf) == [0, 0, 0]                        # empty launch
                    continue
                G = H // Hkv
                rows = 32 * got["waves"]                                 # a wave owns 32 (token, head) rows
                assert got["tile_tokens"] >= 1 and got["tile_tokens"] * G <= rows
                assert got["tile_tokens"] == rows // G                   # no row of the workgroup idle that a token could use
                assert (got["q_tiles"] - 1) * got["tile_tokens"] < n <= got["q_tiles"] * got["tile_tokens"]
                assert got == dict(tile_tokens=128 // G, q_tiles=-(-n // (128 // G)), waves=4)   # every group size 1 .. 8, stated outright
    assert lib.qs_append_attention_plan(1, 4, 8, 3, C.cast(buf, C.c_void_p)) == -1 and list(buf) == [0, 0, 0]
    assert lib.qs_append_attention_plan(1, 4, 18, 2, C.cast(buf, C.c_void_p)) == -2
    assert lib.qs_append_attention_plan(1, 4, 8, 2, None) == -1


@pytest.mark.parametrize("H,Hkv", [(8, 2), (4, 4)])
@pytest.mark.parametrize("past", [1, 130, 200])
def test_composition_with_one_new_token_is_the_decode_oracle(H, Hkv, past):
    """n = 1, KV8: the composition (tests/_append_cases.py) rounded to fp16 is within 1 fp16 ulp of
    oracle.kvattn.decode_attention(mode="fp32") - the same float64 mathematics up to the decode oracle's +1e-6 in the softmax
    denominator.  Pins rule 3 of the semantics (keys < past from the pages, the new token in fp16) to the existing definition."""
    r = np.random.default_rng(100 * H + past)
    B, mb = 2, past // 64 + 2
    tables, nblocks = scattered_tables(r, B, mb)
    pool = kvattn.PagePool(nblocks, Hkv, 128, False, fill=0xFF)
    W = (H + 2 * Hkv) * 128
    # the cache: `past` tokens per sequence through the prefill writer oracle
    ctx = r.standard_normal((B * past, W)).astype(np.float16)
    cu = (np.arange(B + 1) * past).astype(np.int32)
    kvattn.prefill_update_kv_cache(ctx, np.full(B, past), kvattn.compute_padding_offsets(cu, past, B * past), tables, pool, H, Hkv,
                                   past, BASE)
    new = r.standard_normal((B, W)).astype(np.float16)
    cu_q, pasts = np.arange(B + 1, dtype=np.int32), np.full(B, past, np.int32)
    comp = expected(rotate_rows(new, cu_q, pasts, H, Hkv, BASE), cu_q, pasts, tables, pool, H, Hkv).astype(np.float16)
    q = new[:, : H * 128].reshape(B, H, 128)
    k = new[:, H * 128: (H + Hkv) * 128].reshape(B, Hkv, 128)
    v = new[:, (H + Hkv) * 128:].reshape(B, Hkv, 128)
    dec = kvattn.decode_attention(q, k, v, tables, pasts + 1, pool, BASE, mode="fp32")
    assert ulp_diff_f16(comp, dec).max() <= 1
