"""GPU parity of the attention kernels on inputs where a few planted keys decide the output (tests/_attn_cases.py: needles
at every tile / wave / workgroup / unit / page / split boundary, attention sinks, per-tile maximum ramps across the prefill
kernel's lazy-maximum threshold, a maximum confined to one KV split, a dominant or negligible new token, anti-needles past
the sequence end, peaked random scores).  The bars are the existing ones: 2e-3 against the float64 prefill oracle, 1e-3
against kvattn.decode_attention(mode="exact"); tests/test_attn_cases.py proves on the CPU that every case moves by >= 50x
its bar when its planted key is dropped or a masked key leaks."""
import numpy as np
import pytest
import torch

import _attn_cases as A
from _helpers import DevPools, dev

pytestmark = pytest.mark.gpu


@pytest.fixture(params=[0, 1], ids=["round6", "rounds2to5"])
def flash_variant(request):
    """Both key loops of the prefill provider (as in tests/test_flash_gpu.py)."""
    from qserve_amd._lib import lib
    assert lib.qs_debug_flash_variant(request.param) == 0
    yield request.param
    lib.qs_debug_flash_variant(0)


@pytest.mark.parametrize("name", A.PREFILL_CASES)
def test_prefill_planted(gpu, flash_variant, name):
    from flash_attn.flash_attn_interface import flash_attn_varlen_func
    sp = A.prefill(name)
    c = sp["c"]
    H, Hkv = c["H"], c["Hkv"]
    Tq, Tk = int(c["cu_q"][-1]), int(c["cu_k"][-1])
    if sp["packed"]:
        # q, k, v as strided views of one packed qkv buffer, as the reference passes them
        qkv = dev(np.concatenate([c["q"].reshape(Tq, -1), c["k"].reshape(Tk, -1), c["v"].reshape(Tk, -1)], axis=1))
        q, k, v = qkv.split([H * 128, Hkv * 128, Hkv * 128], dim=-1)
        q, k, v = q.reshape(Tq, H, 128), k.reshape(Tk, Hkv, 128), v.reshape(Tk, Hkv, 128)
    else:
        q, k, v = dev(c["q"]), dev(c["k"]), dev(c["v"])
    lq, lk = np.diff(c["cu_q"]), np.diff(c["cu_k"])
    default = abs(c["scale"] - 1.0 / np.sqrt(128.0)) < 1e-12
    out = flash_attn_varlen_func(q, k, v, dev(c["cu_q"]), dev(c["cu_k"]), int(lq.max()), int(lk.max()), dropout_p=0.0,
                                 softmax_scale=None if default else c["scale"], causal=sp["causal"])
    torch.cuda.synchronize()
    o = out.cpu().numpy().astype(np.float64)
    assert np.isfinite(o).all()
    if sp.get("rows") is None:
        ref = A.to_tokens(c, sp["ref"])
    else:
        rows = sp["rows"][0] + int(c["cu_q"][0])
        o, ref = o[rows], sp["ref"][0].transpose(1, 0, 2)
    err = np.abs(o - ref)
    assert err.max() <= A.PREFILL_BAR, f"max abs err {err.max():.2e} at {np.unravel_index(err.argmax(), err.shape)}"
    if "zero_rows" in sp:            # rows that see no key: exactly 0, the oracle's definition
        assert (o[sp["zero_rows"]] == 0).all()


def _decode_inputs(gpu, c):
    B, H, Hkv = c["q"].shape[0], c["H"], c["Hkv"]
    pools = DevPools(c["nblocks"], Hkv, c["int4"], gpu, fill=0)
    pools.k.copy_(torch.from_numpy(c["pool"].k))
    pools.v.copy_(torch.from_numpy(c["pool"].v))
    buf = dev(np.concatenate([c["q"].reshape(B, -1), c["k"].reshape(B, -1), c["v"].reshape(B, -1)], axis=1))
    q, k, v = buf.split([H * 128, Hkv * 128, Hkv * 128], dim=-1)
    return pools, q.reshape(B, H, 128), k.reshape(B, Hkv, 128), v.reshape(B, Hkv, 128)


def _check_decode(sp, out, pools, ref=None):
    o = out.cpu().numpy().astype(np.float32)
    assert np.isfinite(o).all()
    err = np.abs(o - (sp["ref"] if ref is None else ref).astype(np.float32))
    assert err.max() <= A.DECODE_BAR, f"max abs err {err.max():.2e} at {np.unravel_index(err.argmax(), err.shape)}"
    assert np.array_equal(pools.k.cpu().numpy(), sp["pool_after"].k), "K pages differ after the step"
    assert np.array_equal(pools.v.cpu().numpy(), sp["pool_after"].v), "V pages differ after the step"


PLANS = {"default": 0, "split2": 102, "split3": 103, "split7": 107, "valu": 1}


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("name", A.DECODE_CASES)
def test_decode_planted(gpu, name, plan):
    import qserve_backend.fused_attention as fa
    from qserve_amd._lib import lib
    sp = A.decode(name)
    c = sp["c"]
    pools, q, k, v = _decode_inputs(gpu, c)
    spt = c["Hkv"] * (64 if c["int4"] else 128)
    lib.qs_set_attention_variant(PLANS[plan])
    try:
        out = fa.single_query_attention(q, k, v, pools.pointers(c["tables"]), dev(c["lengths"]), None, 8192, 64, spt, c["L"],
                                        128, A.ROPE, True, c["int4"], True)
        torch.cuda.synchronize()
    finally:
        lib.qs_set_attention_variant(0)
    if plan != "valu":
        _check_decode(sp, out, pools)
        return
    # The VALU kernel de-quantises K and V to fp16 exactly as the reference does (attention.hip's header; KV4 hfma2 with a
    # pre-rounded fp16(-scale * zero)) and does everything after it in fp32.  So: within the bar of the attention over
    # THAT cache (kvattn.kv_dequantize mode "kernel", float64 math) ...
    _check_decode(sp, out, pools, ref=A.decode_fp16_cache(name))
    # ... and of the exact one within the bar plus the bound that rounding implies (_attn_cases.dequant_rounding_bound).
    # On the planted cases that bound is < 6e-4 and the plain bar holds; on peaked random scores (|q| ~ 8 sqrt(128)) the
    # rounding alone moves the output by up to ~6e-3, and mode "fp32" (one rounding of scale * (n - zero), no pre-rounded
    # zero term) is a different fp16 cache, ~5e-3 from this one: neither is the VALU kernel's reference.
    o = out.cpu().numpy().astype(np.float64)
    err = np.abs(o - sp["ref"].astype(np.float64))
    if name.startswith("peaked"):
        bound = A.DECODE_BAR + A.decode_rounding_bound(name)
        assert (err <= bound).all(), f"max err / bound {(err / bound).max():.2f}"
    else:
        assert err.max() <= A.DECODE_BAR, f"max abs err vs exact {err.max():.2e}"


@pytest.mark.parametrize("name", [n for n in A.DECODE_CASES if ":kv4" in n])
def test_decode_planted_fused_entry(gpu, name):
    """The decode step's entry (attention + the quantiser of its output in one call), KV4, the planner's own choice."""
    from qserve_amd import fused
    sp = A.decode(name)
    c = sp["c"]
    B, H = c["q"].shape[0], c["H"]
    pools, q, k, v = _decode_inputs(gpu, c)
    qo = torch.empty((B, H * 128), dtype=torch.int8, device=gpu)
    qs = torch.empty((B,), dtype=torch.float16, device=gpu)
    qm = torch.empty((B,), dtype=torch.float16, device=gpu)
    out = fused.single_query_attention_quant(q, k, v, pools.pointers(c["tables"]), dev(c["lengths"]), qo, qs, 8192, 64,
                                             c["Hkv"] * 64, c["L"], 128, A.ROPE, True, True, True, quant_sum=qm)
    torch.cuda.synchronize()
    _check_decode(sp, out, pools)
