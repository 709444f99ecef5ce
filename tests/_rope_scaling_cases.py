"""The numpy restatement of rotation under a RoPE frequency profile (include/qserve_amd.h, qs_rope_profile_register), and the test
profiles.  A profile is (denom float32 [64], mscale float32); the ONE definition of its coefficients is

    ang = float32(pos) / denom[pair];   c = float32(cos(float64(ang))) * mscale;   s = float32(sin(float64(ang))) * mscale

(float32 division, one float32 multiply).  The rotation is oracle.kvattn.rope_neox's, the quantiser kvattn.kv_quantize, the pages
kvattn.PagePool.write_token, attention _append_cases.expected (decode: n = 1, past = L - 1) - nothing else is restated here."""
import numpy as np

from _append_cases import expected, host_pool
from _tree_cases import depths
from oracle import kvattn

LLAMA3 = dict(rope_type="llama3", factor=8.0, low_freq_factor=1.0, high_freq_factor=4.0, original_max_position_embeddings=64)   # base 1e4
YARN = dict(rope_type="yarn", factor=4.0, original_max_position_embeddings=64)      # base 1e4: mscale = 0.1 ln 4 + 1 != 1
BASE = 1e4


def coef(pos, prof):
    denom, mscale = np.asarray(prof[0], np.float32), np.float32(prof[1])
    ang = (np.float32(pos) / denom).astype(np.float32)
    c = (np.cos(ang.astype(np.float64)).astype(np.float32) * mscale).astype(np.float32)
    s = (np.sin(ang.astype(np.float64)).astype(np.float32) * mscale).astype(np.float32)
    return c, s


def rope_neox(x, pos, prof):
    """kvattn.rope_neox with the profile's coefficients: fp32 products and sums without contraction, rounded to fp16."""
    x = np.asarray(x, np.float16)
    c, s = coef(pos, prof)
    a, b = x[..., :64].astype(np.float32), x[..., 64:].astype(np.float32)
    ra = ((c * a).astype(np.float32) - (s * b).astype(np.float32)).astype(np.float32)
    rb = ((c * b).astype(np.float32) + (s * a).astype(np.float32)).astype(np.float32)
    return np.concatenate([ra, rb], axis=-1).astype(np.float16)


def rotate_rows(qkv, cu_q, past, H, Hkv, prof, words=None):
    """The packed buffer after a writer: q and k heads of row i of sequence b rotated at past[b] + i (words: at past[b] + depth of node i)."""
    out = np.array(qkv, np.float16, copy=True)
    for b in range(len(past)):
        s, e = int(cu_q[b]), int(cu_q[b + 1])
        d = depths(words[s:e], e - s) if words is not None else range(e - s)
        for i, t in enumerate(range(s, e)):
            qk = out[t, : (H + Hkv) * 128].reshape(H + Hkv, 128)
            qk[:] = rope_neox(qk, int(past[b]) + int(d[i]), prof)
    return out


def write_rows(pool, src, rot, cu_q, past, tables, H, Hkv):
    """Rows of every sequence into `pool` at positions past[b] + i: K from the rotated rows, V from the source rows."""
    kb, ks, kz = kvattn.kv_quantize(rot[:, H * 128:(H + Hkv) * 128].reshape(-1, Hkv, 128), pool.int4)
    vb, vs, vz = kvattn.kv_quantize(src[:, (H + Hkv) * 128:].reshape(-1, Hkv, 128), pool.int4)
    for b in range(len(past)):
        for i, t in enumerate(range(int(cu_q[b]), int(cu_q[b + 1]))):
            pos = int(past[b]) + i
            for h in range(Hkv):
                pool.write_token("k", int(tables[b, 0, pos // 64]), pos % 64, h, kb[t, h], ks[t, h], kz[t, h])
                pool.write_token("v", int(tables[b, 1, pos // 64]), pos % 64, h, vb[t, h], vs[t, h], vz[t, h])


def history(pool, rng, tables, pasts, H, Hkv, prof):
    """A random past of `pasts[b]` tokens per sequence, rotated under the profile, into `pool` (host only)."""
    for b, p in enumerate(pasts):
        if p:
            ctx = rng.standard_normal((p, (H + 2 * Hkv) * 128)).astype(np.float16)
            cu, z = np.asarray([0, p], np.int32), np.zeros(1, np.int32)
            write_rows(pool, ctx, rotate_rows(ctx, cu, z, H, Hkv, prof), cu, z, tables[b:b + 1], H, Hkv)


def expect_writer(pool0, src, cu_q, past, tables, H, Hkv, prof, words=None):
    """-> (rotated rows, K pool, V pool) after the prefill (past = 0), append or tree (words) writer on pages `pool0`."""
    rot = rotate_rows(src, cu_q, past, H, Hkv, prof, words)
    want = host_pool(pool0.k, pool0.v, Hkv, pool0.int4)
    write_rows(want, src, rot, cu_q, past, tables, H, Hkv)
    return rot, want.k, want.v


def expect_decode(pool0, new, lengths, tables, H, Hkv, prof):
    """-> (float32 out [B, H, 128], K pool, V pool): one new token per sequence at position L - 1 over `pool0`."""
    B = len(lengths)
    cu, past = np.arange(B + 1, dtype=np.int32), np.asarray(lengths, np.int32) - 1
    rot, k, v = expect_writer(pool0, new, cu, past, tables, H, Hkv, prof)
    return expected(rot, cu, past, tables, pool0, H, Hkv).reshape(B, H, 128), k, v
