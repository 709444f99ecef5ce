"""RoPE frequency profiles: llama3, linear and YaRN scaling as 64 denominators and one mscale (include/qserve_amd.h,
qs_rope_profile_register; DESIGN.md "RoPE frequency profiles").

A profile stands in for the rotary base: the kernels and the library's tables evaluate

    ang = float32(pos) / denom[pair];   c = float32(cos(float64(ang))) * mscale;   s = float32(sin(float64(ang))) * mscale

`profile()` computes denom and mscale in float64 from the un-scaled denominators - formed exactly as the kernels form them from a base:
float32 exponent 2i/128, pow in double on the float32 base, rounded to float32 - applies the scaling rule of the type and rounds ONCE to
float32.  The rules are those of transformers' modeling_rope_utils (_compute_linear_scaling_rope_parameters, _compute_llama3_parameters,
_compute_yarn_parameters); types whose frequencies depend on the running length cannot be a fixed profile and are refused."""
import ctypes as C
import math

import numpy as np

PAIRS = 64          # head_dim 128: the only one the kernels rotate
_REFUSED = {
    "dynamic": "its frequencies depend on the current sequence length, a profile is fixed",
    "longrope": "it switches between two factor sets by sequence length, a profile is fixed",
    "proportional": "proportional scaling is not implemented by the kernels' profile",
}


def _type_of(scaling):
    t = scaling.get("rope_type", scaling.get("type"))
    return "default" if t is None else str(t)


def _check_partial(where, value):
    if value is not None and float(value) != 1.0:
        raise ValueError(f"rope scaling: partial_rotary_factor = {value} ({where}) is not supported: the kernels rotate all 128 dimensions")


def scaling_from_hf_config(conf):
    """An HF config.json dict -> (rope_theta, rope_scaling dict or None, original_max_position or None).  Reads `rope_scaling` (with
    `type` or `rope_type`), transformers-5 `rope_parameters` (which carries rope_theta itself), or neither; `default` scaling is None.
    The third value is what `profile` falls back to where the scaling dict has no original_max_position_embeddings.
    ValueError: partial_rotary_factor != 1, a head dimension other than 128, per-layer-type rope_parameters."""
    theta = conf.get("rope_theta")
    scaling = conf.get("rope_scaling")
    params = conf.get("rope_parameters")
    if params is not None:
        if any(isinstance(v, dict) for v in params.values()):
            raise ValueError("rope scaling: per-layer-type rope_parameters are not supported: the engine rotates every layer alike")
        if params.get("rope_theta") is not None:
            theta = params["rope_theta"]
        scaling = {k: v for k, v in params.items() if k != "rope_theta"}
    if theta is None:
        raise ValueError("rope scaling: the config has no rope_theta")
    _check_partial("config", conf.get("partial_rotary_factor"))
    head_dim = conf.get("head_dim")
    if head_dim is None and conf.get("hidden_size") and conf.get("num_attention_heads"):
        head_dim = conf["hidden_size"] // conf["num_attention_heads"]
    if head_dim is not None and int(head_dim) != 2 * PAIRS:
        raise ValueError(f"rope scaling: head dimension {head_dim} is not supported: the kernels rotate head_dim = 128 only")
    if scaling is not None:
        scaling = dict(scaling)
        _check_partial("rope_parameters", scaling.get("partial_rotary_factor"))
        scaling["rope_type"] = _type_of(scaling)
        scaling.pop("type", None)
        if scaling["rope_type"] == "default":
            scaling = None
    return float(theta), scaling, conf.get("max_position_embeddings")


def base_denominators(rope_theta):
    """float32 [64]: what the kernels divide a position by for a plain base (oracle/kvattn.py rope_coef, csrc/kv_quant.h rope_coef)."""
    expo = (np.arange(PAIRS, dtype=np.float32) * np.float32(2.0) / np.float32(2 * PAIRS)).astype(np.float32)
    return np.power(np.float64(np.float32(rope_theta)), expo.astype(np.float64)).astype(np.float32)


def _get_mscale(scale, mscale=1.0):
    return 1.0 if scale <= 1 else 0.1 * mscale * math.log(scale) + 1.0


def _original(scaling, fallback, rtype):
    orig = scaling.get("original_max_position_embeddings", fallback)
    if orig is None:
        raise ValueError(f"rope scaling type {rtype!r}: original_max_position_embeddings is missing")
    return orig


def profile(rope_theta, rope_scaling, original_max_position=None):
    """-> (denom float32 [64], mscale float32) of rope_scaling (a dict with `rope_type` or `type`: linear, llama3, yarn), or None for no
    / `default` scaling: the base itself is then what the kernels take.  ValueError for every other type, with the reason."""
    if rope_scaling is None:
        return None
    rtype = _type_of(rope_scaling)
    if rtype == "default":
        return None
    _check_partial("rope_scaling", rope_scaling.get("partial_rotary_factor"))
    if rtype in _REFUSED:
        raise ValueError(f"rope scaling type {rtype!r} is not supported: {_REFUSED[rtype]}")
    d = base_denominators(rope_theta).astype(np.float64)      # un-scaled, float32 values
    mscale = 1.0
    if rtype == "linear":
        d = d * float(rope_scaling["factor"])
    elif rtype == "llama3":
        factor, low_f, high_f = (float(rope_scaling[k]) for k in ("factor", "low_freq_factor", "high_freq_factor"))
        old = float(_original(rope_scaling, original_max_position, rtype))
        inv = 1.0 / d
        wavelen = 2.0 * math.pi * d
        smooth = (old / wavelen - low_f) / (high_f - low_f)
        blended = (1.0 - smooth) * inv / factor + smooth * inv
        low, high = wavelen > old / low_f, wavelen < old / high_f          # low frequencies: divided by factor; high ones: kept
        d = 1.0 / np.where(low, inv / factor, np.where(high, inv, blended))
    elif rtype == "yarn":
        factor = float(rope_scaling["factor"])
        old = float(_original(rope_scaling, original_max_position, rtype))
        mscale = rope_scaling.get("attention_factor")
        if mscale is None:
            m, m_all = rope_scaling.get("mscale"), rope_scaling.get("mscale_all_dim")
            mscale = float(_get_mscale(factor, m) / _get_mscale(factor, m_all)) if m and m_all else _get_mscale(factor)
        beta_fast, beta_slow = rope_scaling.get("beta_fast") or 32, rope_scaling.get("beta_slow") or 1
        base, dim = float(rope_theta), 2 * PAIRS

        def correction_dim(rotations):
            return (dim * math.log(old / (rotations * 2 * math.pi))) / (2 * math.log(base))

        lo, hi = correction_dim(beta_fast), correction_dim(beta_slow)
        if rope_scaling.get("truncate", True):
            lo, hi = math.floor(lo), math.ceil(hi)
        lo, hi = max(lo, 0), min(hi, dim - 1)
        if lo == hi:
            hi += 0.001
        ramp = np.clip((np.arange(PAIRS, dtype=np.float64) - lo) / (hi - lo), 0.0, 1.0)
        extra = 1.0 - ramp                                                  # 1: extrapolated (kept), 0: interpolated (divided by factor)
        d = 1.0 / ((1.0 / (factor * d)) * (1.0 - extra) + (1.0 / d) * extra)
    else:
        raise ValueError(f"rope scaling type {rtype!r} is not supported: unknown type (supported: default, linear, llama3, yarn)")
    return d.astype(np.float32), np.float32(mscale)


def register(denom, mscale, table_positions):
    """Register the profile on the CURRENT device (qs_rope_profile_register) -> its key, a negative float to pass wherever a rotary base
    is passed.  The same profile gives the same key on every device.  Eager: raises inside a stream capture."""
    import torch
    from ._lib import check, lib
    denom = np.ascontiguousarray(denom, dtype=np.float32)
    if denom.shape != (PAIRS,):
        raise ValueError(f"rope profile: {denom.shape} denominators, expected ({PAIRS},)")
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("qs_rope_profile_register: called inside a stream capture - register before capturing (the table is built eagerly)")
    key = C.c_float(0.0)
    check(lib.qs_rope_profile_register(denom.ctypes.data_as(C.c_void_p), PAIRS, float(np.float32(mscale)), int(table_positions), C.byref(key)),
          "qs_rope_profile_register")
    return float(key.value)


def profile_state(key):
    """(profiles of the process, rows of the longest table of `key` on the current device): qs_debug_rope_profile_state."""
    from ._lib import check, lib
    used, longest = C.c_int(-1), C.c_int(-1)
    check(lib.qs_debug_rope_profile_state(float(key), C.byref(used), C.byref(longest)), "qs_debug_rope_profile_state")
    return used.value, longest.value
