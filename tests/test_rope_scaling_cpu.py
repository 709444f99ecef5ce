"""qserve_amd/rope.py on the host: the profiles of linear, llama3 and YaRN scaling against the installed transformers, the identity of
factor 1, the band populations of the profile the GPU tests use, config parsing, and every refusal with its message.

The bar against transformers (relative 1e-6 on 1 / denom) is about 16 float32 ulps: transformers evaluates a chain of under ten float32
operations, qserve_amd.rope evaluates in float64 and rounds once."""
import math

import numpy as np
import pytest

from oracle import kvattn
from qserve_amd import rope

LLAMA3_CASES = [(5e5, 8.0, 1.0, 4.0, 8192), (1e4, 8.0, 1.0, 4.0, 64), (5e5, 32.0, 1.0, 4.0, 8192)]
YARN_CASES = [dict(factor=4.0), dict(factor=40.0), dict(factor=4.0, mscale=1.0, mscale_all_dim=0.707),
              dict(factor=40.0, mscale=1.0, mscale_all_dim=1.0), dict(factor=40.0, mscale=0.707, mscale_all_dim=1.0)]


def _llama3(factor, low, high, orig):
    return dict(rope_type="llama3", factor=factor, low_freq_factor=low, high_freq_factor=high, original_max_position_embeddings=orig)


def _oracle_denominators(base):
    """What oracle/kvattn.rope_coef divides a position by (its own three lines; the coefficients are compared with it below)."""
    i2 = np.arange(64, dtype=np.float32) * np.float32(2.0)
    expo = (i2 / np.float32(128)).astype(np.float32)
    return np.power(np.float64(np.float32(base)), expo.astype(np.float64)).astype(np.float32)


@pytest.mark.parametrize("base", [1e4, 5e5, 1e6])
def test_linear_factor_one_is_the_identity(base):
    denom, mscale = rope.profile(base, dict(rope_type="linear", factor=1.0))
    want = _oracle_denominators(base)
    assert denom.dtype == np.float32 and np.array_equal(denom.view(np.uint32), want.view(np.uint32))
    assert type(mscale) is np.float32 and mscale == np.float32(1.0)
    assert np.array_equal(rope.base_denominators(base).view(np.uint32), want.view(np.uint32))
    # and the definition of the coefficients with them is the oracle's for the base, bit for bit
    for pos in (0, 1, 63, 1000, 32767):
        ang = (np.float32(pos) / denom).astype(np.float32)
        c, s = kvattn.rope_coef(pos, 128, base)
        assert np.array_equal(np.cos(ang.astype(np.float64)).astype(np.float32).view(np.uint32), c.view(np.uint32))
        assert np.array_equal(np.sin(ang.astype(np.float64)).astype(np.float32).view(np.uint32), s.view(np.uint32))


def test_no_scaling_is_no_profile():
    assert rope.profile(1e4, None) is None
    assert rope.profile(1e4, dict(rope_type="default")) is None and rope.profile(1e4, dict(type="default")) is None


def _transformers(base, scaling):
    mru = pytest.importorskip("transformers.modeling_rope_utils")
    from transformers import LlamaConfig
    params = dict(scaling, rope_theta=base)
    try:
        conf = LlamaConfig(hidden_size=4096, num_attention_heads=32, max_position_embeddings=131072, rope_parameters=params)
    except TypeError:      # transformers 4: rope_theta and rope_scaling are config fields of their own
        conf = LlamaConfig(hidden_size=4096, num_attention_heads=32, max_position_embeddings=131072, rope_theta=base, rope_scaling=dict(scaling))
    inv_freq, attention_factor = mru.ROPE_INIT_FUNCTIONS[scaling["rope_type"]](conf, "cpu")
    return inv_freq.double().numpy(), float(attention_factor)


def _against_transformers(base, scaling):
    inv_freq, attention_factor = _transformers(base, scaling)
    denom, mscale = rope.profile(base, scaling)
    rel = float(np.max(np.abs(1.0 / denom.astype(np.float64) - inv_freq) / inv_freq))
    print(f"{scaling['rope_type']} base {base:g} {scaling}: max relative difference of 1/denom to transformers {rel:.2e}, mscale {mscale!r}")
    assert rel <= 1e-6
    assert mscale == np.float32(attention_factor)
    return mscale


@pytest.mark.parametrize("case", LLAMA3_CASES, ids=lambda c: f"{c[0]:g}-f{c[1]:g}-o{c[4]}")
def test_llama3_against_transformers(case):
    assert _against_transformers(case[0], _llama3(*case[1:])) == np.float32(1.0)


def test_linear_against_transformers():
    assert _against_transformers(1e4, dict(rope_type="linear", factor=4.0)) == np.float32(1.0)


@pytest.mark.parametrize("extra", YARN_CASES, ids=lambda e: "-".join(f"{k[:2]}{v:g}" for k, v in e.items()))
def test_yarn_against_transformers(extra):
    mscale = _against_transformers(1e6, dict(rope_type="yarn", original_max_position_embeddings=32768, **extra))
    if "mscale" not in extra:
        assert mscale == np.float32(0.1 * math.log(extra["factor"]) + 1.0) and mscale != np.float32(1.0)


def test_gpu_profile_populates_every_llama3_band():
    """(1e4, 8, 1, 4, 64), the profile of the GPU tests: 47 pairs divided by the factor, 10 blended, 7 kept - every branch is exercised."""
    base, (factor, low, high, orig) = 1e4, (8.0, 1.0, 4.0, 64)
    denom, _ = rope.profile(base, _llama3(factor, low, high, orig))
    plain = rope.base_denominators(base)
    kept = denom == plain
    scaled = denom == (plain.astype(np.float64) * factor).astype(np.float32)
    assert int(kept.sum()) == 7 and int(scaled.sum()) == 47 and int((~kept & ~scaled).sum()) == 10
    # the bands are contiguous: high frequencies (short wavelengths) first
    assert kept[:7].all() and scaled[17:].all()
    blended = denom[7:17].astype(np.float64) / plain[7:17]
    assert (blended > 1.0).all() and (blended < factor).all() and (np.diff(blended) > 0).all()
    # the yarn profile of the GPU tests has an mscale that is not 1
    assert rope.profile(1e4, dict(rope_type="yarn", factor=4.0, original_max_position_embeddings=64))[1] != np.float32(1.0)


def test_original_max_position_falls_back_to_the_argument():
    s = _llama3(8.0, 1.0, 4.0, 8192)
    t = {k: v for k, v in s.items() if k != "original_max_position_embeddings"}
    a, b = rope.profile(5e5, s), rope.profile(5e5, t, 8192)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]
    with pytest.raises(ValueError, match="original_max_position_embeddings is missing"):
        rope.profile(5e5, t)


HF = dict(hidden_size=4096, num_attention_heads=32, max_position_embeddings=131072)


def test_config_spellings():
    s = dict(factor=8.0, low_freq_factor=1.0, high_freq_factor=4.0, original_max_position_embeddings=8192)
    want = dict(s, rope_type="llama3")
    assert rope.scaling_from_hf_config(dict(HF, rope_theta=5e5, rope_scaling=dict(s, rope_type="llama3"))) == (5e5, want, 131072)
    assert rope.scaling_from_hf_config(dict(HF, rope_theta=5e5, rope_scaling=dict(s, type="llama3"))) == (5e5, want, 131072)
    assert rope.scaling_from_hf_config(dict(HF, rope_parameters=dict(s, rope_type="llama3", rope_theta=5e5))) == (5e5, want, 131072)
    assert rope.scaling_from_hf_config(dict(HF, rope_theta=1e4)) == (1e4, None, 131072)
    assert rope.scaling_from_hf_config(dict(HF, rope_theta=1e4, rope_scaling=None)) == (1e4, None, 131072)
    assert rope.scaling_from_hf_config(dict(HF, rope_parameters=dict(rope_type="default", rope_theta=1e6))) == (1e6, None, 131072)
    assert rope.scaling_from_hf_config(dict(rope_theta=1e4, head_dim=128, hidden_size=2048, num_attention_heads=32))[1] is None
    theta, scaling, orig = rope.scaling_from_hf_config(dict(HF, rope_theta=1e6, rope_scaling=dict(type="yarn", factor=4.0)))
    assert rope.profile(theta, scaling, orig)[1] == np.float32(0.1 * math.log(4.0) + 1.0)


@pytest.mark.parametrize("rtype,reason", [("dynamic", "depend on the current sequence length"), ("longrope", "two factor sets"),
                                          ("proportional", "not implemented"), ("ntk-by-parts", "unknown type")])
def test_refused_types(rtype, reason):
    for key in ("rope_type", "type"):
        with pytest.raises(ValueError, match=reason) as e:
            rope.profile(1e4, {key: rtype, "factor": 2.0})
        assert repr(rtype) in str(e.value)


def test_refused_partial_rotary_and_head_dim():
    with pytest.raises(ValueError, match="partial_rotary_factor = 0.5"):
        rope.scaling_from_hf_config(dict(HF, rope_theta=1e4, partial_rotary_factor=0.5))
    with pytest.raises(ValueError, match="partial_rotary_factor = 0.25"):
        rope.scaling_from_hf_config(dict(HF, rope_parameters=dict(rope_type="linear", factor=2.0, rope_theta=1e4, partial_rotary_factor=0.25)))
    with pytest.raises(ValueError, match="partial_rotary_factor = 0.5"):
        rope.profile(1e4, dict(rope_type="linear", factor=2.0, partial_rotary_factor=0.5))
    with pytest.raises(ValueError, match="head dimension 64"):
        rope.scaling_from_hf_config(dict(rope_theta=1e4, hidden_size=2048, num_attention_heads=32))
    with pytest.raises(ValueError, match="head dimension 96"):
        rope.scaling_from_hf_config(dict(HF, rope_theta=1e4, head_dim=96))
    with pytest.raises(ValueError, match="per-layer-type"):
        rope.scaling_from_hf_config(dict(HF, rope_parameters=dict(full_attention=dict(rope_type="default", rope_theta=1e4))))
    assert rope.scaling_from_hf_config(dict(HF, rope_theta=1e4, partial_rotary_factor=1.0))[1] is None


def test_engine_configs():
    from qserve_amd.decode import LLAMA3_8B, LLAMA31_8B
    s = LLAMA31_8B["rope_scaling"]
    assert (s["rope_type"], s["factor"], s["low_freq_factor"], s["high_freq_factor"], s["original_max_position_embeddings"]) == ("llama3", 8, 1, 4, 8192)
    assert {k: v for k, v in LLAMA31_8B.items() if k not in ("name", "rope_scaling")} == {k: v for k, v in LLAMA3_8B.items() if k != "name"}
    assert "rope_scaling" not in LLAMA3_8B


def test_restatement_with_the_identity_profile_is_the_oracle():
    """tests/_rope_scaling_cases.py under linear factor 1 gives the bytes of the oracle's writers for the base: rows and pages."""
    import _rope_scaling_cases as RC
    from _append_cases import rotate_rows, scattered_tables
    from _tree_cases import rotate_rows_tree, words_from_parents
    r = np.random.default_rng(0)
    H, Hkv, base = 4, 2, 1e4
    prof = rope.profile(base, dict(rope_type="linear", factor=1.0))
    cu, past = np.asarray([0, 5, 8], np.int32), np.asarray([63, 1000], np.int32)
    src = r.standard_normal((8, (H + 2 * Hkv) * 128)).astype(np.float16)
    words = words_from_parents([-1, 0, 0, 1, 3]) + words_from_parents([-1, 0, 0])
    assert np.array_equal(RC.rotate_rows(src, cu, past, H, Hkv, prof).view(np.uint16), rotate_rows(src, cu, past, H, Hkv, base).view(np.uint16))
    assert np.array_equal(RC.rotate_rows(src, cu, past, H, Hkv, prof, words).view(np.uint16),
                          rotate_rows_tree(src, cu, past, words, H, Hkv, base).view(np.uint16))
    for int4 in (True, False):
        tables, nblocks = scattered_tables(r, 1, 3)
        lens = np.asarray([70], np.int32)
        ctx = r.standard_normal((70, (H + 2 * Hkv) * 128)).astype(np.float16)
        want = kvattn.PagePool(nblocks, Hkv, 128, int4, fill=0xFF)
        wrows = ctx.copy()
        kvattn.prefill_update_kv_cache(wrows, lens, np.zeros(70, np.int32), tables, want, H, Hkv, 70, base)
        rot, k, v = RC.expect_writer(kvattn.PagePool(nblocks, Hkv, 128, int4, fill=0xFF), ctx, np.asarray([0, 70], np.int32), np.zeros(1, np.int32),
                                     tables, H, Hkv, prof)
        assert np.array_equal(rot.view(np.uint16), wrows.view(np.uint16)) and np.array_equal(k, want.k) and np.array_equal(v, want.v)


def test_register_argument_validation_without_gpu(built_lib):
    """QS_EINVAL with a message before any device call."""
    import ctypes
    from qserve_amd._lib import lib
    d = rope.base_denominators(1e4)
    key = ctypes.c_float(0.0)
    ptr = d.ctypes.data_as(ctypes.c_void_p)
    assert lib.qs_rope_profile_register(None, 64, 1.0, 64, ctypes.byref(key)) == -1 and b"null pointer" in lib.qs_last_error()
    assert lib.qs_rope_profile_register(ptr, 64, 1.0, 64, None) == -1
    assert lib.qs_rope_profile_register(ptr, 32, 1.0, 64, ctypes.byref(key)) == -1 and b"pairs=32" in lib.qs_last_error()
    for rows in (0, -5, 32769):
        assert lib.qs_rope_profile_register(ptr, 64, 1.0, rows, ctypes.byref(key)) == -1 and b"table_positions" in lib.qs_last_error()
    for m in (0.0, -1.0, float("inf"), float("nan")):
        assert lib.qs_rope_profile_register(ptr, 64, m, 64, ctypes.byref(key)) == -1 and b"mscale" in lib.qs_last_error()
    bad = d.copy()
    bad[17] = 0.0
    assert lib.qs_rope_profile_register(bad.ctypes.data_as(ctypes.c_void_p), 64, 1.0, 64, ctypes.byref(key)) == -1
    assert b"denom[17]" in lib.qs_last_error() and key.value == 0.0
    rows = ctypes.c_int(-1)
    assert lib.qs_debug_rope_profile_state(-1.0, None, ctypes.byref(rows)) == -1
    with pytest.raises(ValueError, match="expected \\(64,\\)"):
        rope.register(d[:32], 1.0, 64)
