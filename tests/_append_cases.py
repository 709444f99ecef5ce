"""Expected values of append attention, composed from the EXISTING oracles (no new oracle arithmetic):

for sequence b with `past` tokens in its pages and n new rows, the keys / values of KV head h are
    kv_dequantize(pool.read_tokens(...)[: past], mode="kernel")   ++   the chunk's rotated k / raw v (fp16)
and oracle.flash.attention_varlen(q_rot, K, V, cu_q, cu_k, causal=True) with len_k = past + n: its bottom-right aligned mask
(j <= i + len_k - len_q) is exactly "row i sees keys 0 .. past + i"."""
import numpy as np

from oracle import flash as oflash
from oracle import kvattn


def host_pool(k_bytes, v_bytes, hkv, int4):
    """uint8 [nblocks, page_bytes] images of a K and a V pool (numpy) -> oracle PagePool over copies of them."""
    pool = kvattn.PagePool(k_bytes.shape[0], hkv, 128, int4)
    assert pool.pb == k_bytes.shape[1] == v_bytes.shape[1]
    pool.k[:] = k_bytes
    pool.v[:] = v_bytes
    return pool


def rotate_rows(qkv, cu_q, past, H, Hkv, rope_base):
    """What the writer leaves in the packed buffer: q and k heads of new token i of sequence b rotated at past[b] + i."""
    out = np.array(qkv, np.float16, copy=True)
    for b in range(len(past)):
        for i, t in enumerate(range(int(cu_q[b]), int(cu_q[b + 1]))):
            qk = out[t, : (H + Hkv) * 128].reshape(H + Hkv, 128)
            qk[:] = kvattn.rope_neox(qk, int(past[b]) + i, rope_base)
    return out


def compose(qkv_rot, cu_q, past, tables, pool, H, Hkv):
    """-> q [T, H, 128], K, V [sum(past + n), Hkv, 128] fp16, cu_k: the inputs of the flash oracle (and of the flash provider)."""
    T = qkv_rot.shape[0]
    q = qkv_rot[:, : H * 128].reshape(T, H, 128)
    k_new = qkv_rot[:, H * 128: (H + Hkv) * 128].reshape(T, Hkv, 128)
    v_new = qkv_rot[:, (H + Hkv) * 128:].reshape(T, Hkv, 128)
    Ks, Vs, cu_k = [], [], [0]
    for b in range(len(past)):
        p, s, e = int(past[b]), int(cu_q[b]), int(cu_q[b + 1])
        Kp = np.zeros((p, Hkv, 128), np.float16)
        Vp = np.zeros((p, Hkv, 128), np.float16)
        for h in range(Hkv):
            kq, ksc, kzr = pool.read_tokens("k", tables[b, 0], h, p)
            vq, vsc, vzr = pool.read_tokens("v", tables[b, 1], h, p)
            Kp[:, h] = kvattn.kv_dequantize(kq, ksc, kzr, pool.int4, mode="kernel")
            Vp[:, h] = kvattn.kv_dequantize(vq, vsc, vzr, pool.int4, mode="kernel")
        Ks += [Kp, k_new[s:e]]
        Vs += [Vp, v_new[s:e]]
        cu_k.append(cu_k[-1] + p + (e - s))
    return (np.ascontiguousarray(q), np.concatenate(Ks).astype(np.float16), np.concatenate(Vs).astype(np.float16),
            np.asarray(cu_k, np.int32))


def expected(qkv_rot, cu_q, past, tables, pool, H, Hkv):
    """float32 [T, H, 128]: append attention of the already rotated rows over `pool` (state BEFORE or AFTER the writer: only
    positions < past are read)."""
    q, K, V, cu_k = compose(qkv_rot, cu_q, past, tables, pool, H, Hkv)
    return oflash.attention_varlen(q, K, V, np.asarray(cu_q, np.int32), cu_k, causal=True)


def expected_rows(qkv_rot, cu_q, past, tables, pool, H, Hkv, rows, heads):
    """The same for sampled (global query row, head) pairs: float32 [len(rows), len(heads), 128]."""
    q, K, V, cu_k = compose(qkv_rot, cu_q, past, tables, pool, H, Hkv)
    return oflash.attention_rows(q, K, V, np.asarray(cu_q, np.int32), cu_k, rows, heads, causal=True)


def scattered_tables(rng, batch, max_blocks, spare=3):
    """Block tables [batch, 2, max_blocks] over a pool of batch * max_blocks + spare blocks, K and V permuted independently;
    the `spare` blocks belong to nobody (canaries).  -> (tables int64, nblocks)"""
    nblocks = batch * max_blocks + spare
    tables = np.stack([rng.permutation(nblocks)[: batch * max_blocks].reshape(batch, max_blocks),
                       rng.permutation(nblocks)[: batch * max_blocks].reshape(batch, max_blocks)], axis=1).astype(np.int64)
    return tables, nblocks
