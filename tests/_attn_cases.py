"""Attention inputs where a few PLANTED keys decide the output (needles, sinks, per-tile maximum ramps, anti-needles), with
float64 references that can also drop a planted key or admit a masked one (the sensitivity check: a case whose answer does
not move when its planted key is removed or a masked key leaks cannot tell a right kernel from a wrong one).

Plain numpy, seeded; shared by tests/test_attn_cases.py (CPU: the builders against the oracles) and the GPU parity tests
tests/test_attn_peaked_gpu.py.

Score design.  Per (sequence, KV head) a sign pattern u in {-1, +1}^128; every query row of the group is s*u plus a little
noise, a planted key is a*u, background keys are small noise.  The score of a planted key is then a*s*128*scale (``level``,
in nats above a background whose scores are ~N(0, 0.3^2)); its value row is a distinct +-0.75 sign pattern, background value
rows are U(-0.25, 0.25), so letting a planted key in or out moves the output by ~0.5.  Sign-pattern keys and values are
two-level vectors: the per-token KV4 / KV8 quantiser stores them almost exactly.  Every check uses the scores the fp16
(and, for decode, quantised) inputs actually reach, never the design."""
import copy
import functools

import numpy as np

from oracle import flash as oflash
from oracle import kvattn

D = 128
LOG2E = 1.4426950408889634
ROPE = 5e5
BN = 64            # key tile of the prefill kernel (qserve_amd/csrc/flash_prefill.hip)
LAZY = 8.0         # its lazy running maximum moves only for a tile more than 2^8 above it


def _sign(r, n=D):
    return np.where(r.random(n) < 0.5, -1.0, 1.0)


# ---------------------------------------------------------------------------------------------------------------------
# prefill (flash_attn_varlen_func): no RoPE, plain fp16 q / k / v
# ---------------------------------------------------------------------------------------------------------------------
def prefill_case(lens_q, lens_k, H, Hkv, planted, seed, s=2.0, scale=None, qnoise=0.05, knoise=0.15, vbg=0.25):
    """planted: {(b, key_in_seq): level_nats} - the same key of every KV head of sequence b (each KV head its own pattern).
    Returns dict(q, k, v [T, heads, 128] fp16, cu_q, cu_k, scale, planted, H, Hkv)."""
    r = np.random.default_rng(seed)
    scale = 1.0 / np.sqrt(D) if scale is None else float(scale)
    G = H // Hkv
    lens_q, lens_k = list(lens_q), list(lens_k)
    cu_q = np.concatenate([[0], np.cumsum(lens_q)]).astype(np.int32)
    cu_k = np.concatenate([[0], np.cumsum(lens_k)]).astype(np.int32)
    Tq, Tk = int(cu_q[-1]), int(cu_k[-1])
    q = np.zeros((Tq, H, D)); k = r.normal(0.0, knoise, (Tk, Hkv, D)); v = r.uniform(-vbg, vbg, (Tk, Hkv, D))
    U = [_sign(r) for _ in range(Hkv)]      # shared by the sequences: a neighbour's planted key scores high here too
    for b in range(len(lens_q)):
        for hk in range(Hkv):
            u = U[hk]
            for g in range(G):
                q[cu_q[b]:cu_q[b + 1], hk * G + g] = s * u + r.normal(0.0, qnoise, (lens_q[b], D))
            for (pb, j), level in planted.items():
                if pb == b:
                    k[cu_k[b] + j, hk] = level / (s * D * scale) * u
                    v[cu_k[b] + j, hk] = 0.75 * _sign(r)
    return dict(q=q.astype(np.float16), k=k.astype(np.float16), v=v.astype(np.float16), cu_q=cu_q, cu_k=cu_k, scale=scale,
                planted=dict(planted), H=H, Hkv=Hkv)


def ramp_case(L, H, Hkv, r_log2, seed, base=4.0, s=4.0, qnoise=0.005):
    """One sequence of L keys: tile t (64 keys) holds one planted key at base + r_log2 * t log2 units above the background, so
    every row's maximum grows by r_log2 per tile it sees."""
    planted = {(0, BN * t + (7 * t + 5) % BN): (base + r_log2 * t) / LOG2E for t in range(L // BN)}
    return prefill_case([L], [L], H, Hkv, planted, seed, s=s, qnoise=qnoise)


def peaked_prefill_case(lens_q, lens_k, H, Hkv, sigma, seed):
    """q ~ N(0, sigma^2), k ~ N(0, 1), v ~ U(-1, 1): random, but a row's softmax is dominated by its top keys."""
    r = np.random.default_rng(seed)
    cu_q = np.concatenate([[0], np.cumsum(lens_q)]).astype(np.int32)
    cu_k = np.concatenate([[0], np.cumsum(lens_k)]).astype(np.int32)
    return dict(q=(sigma * r.standard_normal((int(cu_q[-1]), H, D))).astype(np.float16),
                k=r.standard_normal((int(cu_k[-1]), Hkv, D)).astype(np.float16),
                v=r.uniform(-1, 1, (int(cu_k[-1]), Hkv, D)).astype(np.float16), cu_q=cu_q, cu_k=cu_k, scale=1.0 / np.sqrt(D),
                planted={}, H=H, Hkv=Hkv)


def _seq_scores(c, b, rows, causal):
    """float64 scores [H, len(rows), lk] of sequence b (masked keys -inf) and the visibility mask [len(rows), lk]."""
    q, k = c["q"], c["k"]
    G = c["H"] // c["Hkv"]
    qs, ks = int(c["cu_q"][b]), int(c["cu_k"][b])
    lq, lk = int(c["cu_q"][b + 1]) - qs, int(c["cu_k"][b + 1]) - ks
    rows = np.arange(lq) if rows is None else np.asarray(rows)
    Q = q[qs + rows].astype(np.float64)                                   # [r, H, D]
    K = np.repeat(k[ks:ks + lk].astype(np.float64), G, axis=1)            # [lk, H, D]
    S = np.matmul(Q.transpose(1, 0, 2), K.transpose(1, 2, 0)) * c["scale"]
    vis = np.ones((len(rows), lk), bool)
    if causal:
        vis = np.arange(lk)[None, :] <= rows[:, None] + (lk - lq)
    return S, vis, rows


def prefill_ref(c, causal, rows=None, drop=(), admit=(), only=None):
    """float64 attention of the case -> {b: [H, rows, D]}.
    drop: (b, key) pairs taken out of sequence b.
    admit: (b, global_key, where) - a key that must NOT reach sequence b, let in: where="diag" is a causally masked key of b
    itself, "after" / "before" a neighbour's key read past the end / before the start of b.  It becomes visible to the rows
    a one-key error would show it to: every row without a mask; with one, the rows whose diagonal moved by one reaches it.
    only: the sequences to compute (the others are left out of the result)."""
    q, k, v = c["q"], c["k"], c["v"]
    G = c["H"] // c["Hkv"]
    out = {}
    for b in range(len(c["cu_q"]) - 1):
        rb = None if rows is None else rows.get(b)
        if (rows is not None and rb is None) or (only is not None and b not in only):
            continue
        S, vis, rr = _seq_scores(c, b, rb, causal)
        ks, lk = int(c["cu_k"][b]), int(c["cu_k"][b + 1] - c["cu_k"][b])
        lq = int(c["cu_q"][b + 1] - c["cu_q"][b])
        Vs = np.repeat(v[ks:ks + lk].astype(np.float64), G, axis=1)       # [lk, H, D]
        for (db, j) in drop:
            if db == b:
                vis[:, j] = False
        for (ab, gk, where) in admit:
            if ab != b:
                continue
            if where == "diag":
                j = gk - ks
                vis[:, j] |= (rr + (lk - lq) + 1 >= j) if causal else True
                continue
            kx = np.repeat(k[gk:gk + 1].astype(np.float64), G, axis=1)
            sx = np.matmul(q[int(c["cu_q"][b]) + rr].astype(np.float64).transpose(1, 0, 2), kx.transpose(1, 2, 0)) * c["scale"]
            vx = np.ones((len(rr), 1), bool)
            if causal and where == "after":
                vx[:, 0] = rr + (lk - lq) + 1 >= lk
            S = np.concatenate([sx, S] if where == "before" else [S, sx], axis=2)
            vis = np.concatenate([vx, vis] if where == "before" else [vis, vx], axis=1)
            vv = np.repeat(v[gk:gk + 1].astype(np.float64), G, axis=1)
            Vs = np.concatenate([vv, Vs] if where == "before" else [Vs, vv], axis=0)
        S = np.where(vis[None], S, -np.inf)
        m = S.max(axis=2, keepdims=True) if S.shape[2] else np.zeros(S.shape[:2] + (1,))
        m = np.where(np.isfinite(m), m, 0.0)
        P = np.exp(S - m)
        l = P.sum(axis=2, keepdims=True)
        O = np.matmul(P, Vs.transpose(1, 0, 2)) if S.shape[2] else np.zeros(S.shape[:2] + (D,))
        out[b] = np.where(l > 0, O / np.where(l > 0, l, 1.0), 0.0)
    return out


def to_tokens(c, ref):
    """{b: [H, lq, D]} over all rows -> [Tq, H, D] (the kernel's layout)."""
    o = np.zeros((int(c["cu_q"][-1]), c["H"], D))
    for b, x in ref.items():
        o[int(c["cu_q"][b]):int(c["cu_q"][b + 1])] = x.transpose(1, 0, 2)
    return o


def oracle_prefill(c, causal):
    return oflash.attention_varlen(c["q"], c["k"], c["v"], c["cu_q"], c["cu_k"], scale=c["scale"], causal=causal)


def reached_gaps(c, causal, rows=None):
    """Per sequence: [H, rows] gap in nats between each planted key (the largest one the row sees) and the best other key
    the row sees (nan where the row sees no planted key)."""
    gaps = {}
    for b in range(len(c["cu_q"]) - 1):
        rb = None if rows is None else rows.get(b)
        if rows is not None and rb is None:
            continue
        S, vis, rr = _seq_scores(c, b, rb, causal)
        pl = sorted(j for (pb, j) in c["planted"] if pb == b)
        if not pl or S.shape[2] == 0:
            continue
        S = np.where(vis[None], S, -np.inf)
        isp = np.zeros(S.shape[2], bool); isp[pl] = True
        top = np.where(isp[None, None], S, -np.inf).max(axis=2)
        rest = np.where(isp[None, None], -np.inf, S).max(axis=2)
        gaps[b] = np.where(np.isfinite(top), top - rest, np.nan)
    return gaps


def lazy_rescales(c, causal, b=0):
    """The round-6 key loop's lazy maximum on the REACHED scores (log2 units, 64-key tiles, the rows' visible keys):
    -> (rescales [H, lq]: tiles after a row's first whose maximum exceeded the reference maximum by more than 8 - the O
    accumulators are non-zero and get multiplied by alpha < 1 -, max_p [H, lq]: the largest 2^(score - reference maximum) the
    kernel rounds to fp16, min_alpha [H, lq]: the smallest such alpha)."""
    S, vis, _ = _seq_scores(c, b, None, causal)
    S = np.where(vis[None], S * LOG2E, -np.inf)
    lk = S.shape[2]
    m_run = np.full(S.shape[:2], -np.inf)
    cnt = np.zeros(S.shape[:2], int)
    pmax = np.zeros(S.shape[:2])
    amin = np.ones(S.shape[:2])
    for t in range((lk + BN - 1) // BN):
        mx = S[:, :, t * BN:(t + 1) * BN].max(axis=2)
        move = mx > m_run + LAZY
        later = np.isfinite(m_run) & move
        cnt += later
        amin = np.where(later, np.minimum(amin, np.exp2(m_run - mx)), amin)
        m_run = np.where(move, mx, m_run)
        pmax = np.where(np.isfinite(mx), np.maximum(pmax, np.exp2(mx - m_run)), pmax)
    return cnt, pmax, amin


def top_key_change(c, causal):
    """Per (row, head): max |O - O without that row's top key| (float64) over the whole batch -> [Tq, H]."""
    v = c["v"]
    G = c["H"] // c["Hkv"]
    res = np.zeros((int(c["cu_q"][-1]), c["H"]))
    for b in range(len(c["cu_q"]) - 1):
        S, vis, rr = _seq_scores(c, b, None, causal)
        if S.shape[1] == 0 or S.shape[2] == 0:
            continue
        ks, lk = int(c["cu_k"][b]), S.shape[2]
        Vs = np.repeat(v[ks:ks + lk].astype(np.float64), G, axis=1)
        S = np.where(vis[None], S, -np.inf)
        jt = S.argmax(axis=2)
        P = np.exp(S - S.max(axis=2, keepdims=True))
        O = np.matmul(P, Vs.transpose(1, 0, 2)) / P.sum(axis=2, keepdims=True)
        np.put_along_axis(P, jt[..., None], 0.0, axis=2)
        l2 = P.sum(axis=2, keepdims=True)
        O2 = np.matmul(P, Vs.transpose(1, 0, 2)) / np.where(l2 > 0, l2, 1.0)
        res[int(c["cu_q"][b]):int(c["cu_q"][b + 1])] = np.abs(O2 - O).max(axis=2).T
    return res


# ---------------------------------------------------------------------------------------------------------------------
# decode (single_query_attention): post-RoPE q / k, quantised KV4 / KV8 history written straight into the pages
# ---------------------------------------------------------------------------------------------------------------------
def split_boundaries(L, nsplit, int4):
    """First and last cached token of every split of a context of L tokens (L - 1 cached): the KV4 kernel splits 32-token
    units (attention_mfma.hip), the KV8 kernel 64-token pages (attention_mfma8.hip), ceil(n / nsplit) per split."""
    tl, unit = L - 1, (32 if int4 else 64)
    n = (tl + unit - 1) // unit
    per = (n + nsplit - 1) // nsplit
    out = []
    for z in range(nsplit):
        a, e = z * per, min(n, z * per + per)
        if a < e:
            out += [a * unit, min(e * unit, tl) - 1]
    return out


def decode_case(B, H, Hkv, L, int4, planted, seed, s=2.0, anti=(), qnoise=0.05, knoise=0.15, vbg=0.25, sigma_q=None):
    """planted: {(b, hk, pos): level_nats}; pos < L - 1 is a cached token, pos == L - 1 the new token (its un-rotated k is
    rope_neox_inv of the designed rotated vector).  anti: (b, hk, slot, level) - a finite key with a valid scale / zero in a
    slot of the last page PAST the sequence end.  sigma_q: peaked random instead (q ~ N(0, sigma_q^2) before RoPE,
    history k ~ N(0, 1), v ~ U(-1, 1), no planted keys).
    Returns q, k, v [B, heads, 128] fp16 (the kernel's inputs), tables [B, 2, mb], lengths, pool (oracle PagePool holding
    the cache BEFORE the step), nblocks, mb."""
    r = np.random.default_rng(seed)
    G = H // Hkv
    tl = L - 1
    lengths = np.full(B, L, np.int32)
    mb = (L + 63) // 64
    nblocks = B * mb + 2
    tables = np.zeros((B, 2, mb), np.int64)
    pk, pv = r.permutation(nblocks), r.permutation(nblocks)
    for b in range(B):
        tables[b, 0], tables[b, 1] = pk[b * mb:(b + 1) * mb], pv[b * mb:(b + 1) * mb]
    pool = kvattn.PagePool(nblocks, Hkv, D, int4, fill=0)
    q = np.zeros((B, H, D), np.float16); k = np.zeros((B, Hkv, D), np.float16); v = np.zeros((B, Hkv, D), np.float16)
    a_of = lambda level: level / (s * np.sqrt(D))                       # noqa: E731  (score = a s sqrt(128))
    for b in range(B):
        if sigma_q is not None:
            qr = sigma_q * r.standard_normal((H, D))
            K = r.standard_normal((tl, Hkv, D)); V = r.uniform(-1, 1, (tl, Hkv, D))
            kr_new = r.standard_normal((Hkv, D)); v_new = r.uniform(-1, 1, (Hkv, D))
        else:
            U = np.stack([_sign(r) for _ in range(Hkv)])                  # [Hkv, D]
            qr = np.repeat(s * U, G, axis=0) + r.normal(0, qnoise, (H, D))
            K = r.normal(0, knoise, (tl, Hkv, D)); V = r.uniform(-vbg, vbg, (tl, Hkv, D))
            kr_new = r.normal(0, knoise, (Hkv, D)); v_new = r.uniform(-vbg, vbg, (Hkv, D))
            for (pb, hk, pos), level in planted.items():
                if pb != b:
                    continue
                if pos == tl:
                    kr_new[hk] = a_of(level) * U[hk]; v_new[hk] = 0.75 * _sign(r)
                else:
                    K[pos, hk] = a_of(level) * U[hk]; V[pos, hk] = 0.75 * _sign(r)
        q[b] = kvattn.rope_neox_inv(qr.astype(np.float16), tl, ROPE)
        k[b] = kvattn.rope_neox_inv(kr_new.astype(np.float16), tl, ROPE)
        v[b] = v_new.astype(np.float16)
        for which, X, col in (("k", K, 0), ("v", V, 1)):
            qb, sc, zr = kvattn.kv_quantize(X.astype(np.float16), int4)   # [tl, Hkv, dhb], [tl, Hkv]
            for p in range((tl + 63) // 64):
                data, scv, zrv = pool._views(pool.k if which == "k" else pool.v, int(tables[b, col, p]))
                n = min(64, tl - 64 * p)
                data[:, :n] = qb[64 * p:64 * p + n].transpose(1, 0, 2)
                scv[:, :n] = sc[64 * p:64 * p + n].T
                zrv[:, :n] = zr[64 * p:64 * p + n].T
        if sigma_q is None:
            for (ab, hk, slot, level) in anti:
                if ab != b:
                    continue
                assert tl < slot < mb * 64, "an anti-needle goes into an unused slot of the last page"
                for which, X, col in (("k", a_of(level) * U[hk], 0), ("v", 0.75 * _sign(r), 1)):
                    qb, sc, zr = kvattn.kv_quantize(X.astype(np.float16), int4)
                    pool.write_token(which, int(tables[b, col, slot // 64]), slot % 64, hk, qb, sc, zr)
    return dict(q=q, k=k, v=v, tables=tables, lengths=lengths, pool=pool, nblocks=nblocks, mb=mb, H=H, Hkv=Hkv, L=L,
                int4=int4, planted=dict(planted), anti=list(anti))


def oracle_decode(c, mode="exact"):
    """kvattn.decode_attention(mode) on a copy of the pool -> (out fp16 [B, H, D], pool after the step)."""
    pool = copy.deepcopy(c["pool"])
    out = kvattn.decode_attention(c["q"], c["k"], c["v"], c["tables"], c["lengths"], pool, ROPE, mode)
    return out, pool


def decode_exact(c, drop=(), admit=(), only=None, deq="exact"):
    """The exact oracle's definition restated with edits, float64 -> (out [B, H, D], scores [B, H, L + extra] in nats, the
    new token's last).  drop: (b, hk, pos) taken out (pos == L - 1: the new token).  admit: (b, hk, slot) - a slot past
    the sequence end let in.  only: the sequences to compute (the others stay 0).  deq: kvattn.kv_dequantize's mode for the
    cache ("kernel": the fp16 values the VALU kernel computes, the rest of the math stays float64)."""
    pool, int4 = c["pool"], c["int4"]
    B, H, _ = c["q"].shape
    Hkv = c["Hkv"]
    G = H // Hkv
    out = np.zeros((B, H, D)); scores = {}
    for b in range(B) if only is None else sorted(only):
        tl = int(c["lengths"][b]) - 1
        qr = kvattn.rope_neox(c["q"][b], tl, ROPE).astype(np.float64)
        kr = kvattn.rope_neox(c["k"][b], tl, ROPE).astype(np.float64)
        for hk in range(Hkv):
            extra = sorted(sl for (ab, ah, sl) in admit if ab == b and ah == hk)
            kq, ksc, kzr = pool.read_tokens("k", c["tables"][b, 0], hk, tl + 1 + (max(extra) - tl if extra else 0))
            vq, vsc, vzr = pool.read_tokens("v", c["tables"][b, 1], hk, tl + 1 + (max(extra) - tl if extra else 0))
            Kd = kvattn.kv_dequantize(kq, ksc, kzr, int4, deq).astype(np.float64)
            Vd = kvattn.kv_dequantize(vq, vsc, vzr, int4, deq).astype(np.float64)
            Kall = np.concatenate([Kd[:tl], kr[hk][None], Kd[extra]])
            Vall = np.concatenate([Vd[:tl], c["v"][b, hk][None].astype(np.float64), Vd[extra]])
            keep = np.ones(len(Kall), bool)
            for (db, dh, pos) in drop:
                if db == b and dh == hk:
                    keep[pos] = False
            for g in range(G):
                h = hk * G + g
                sc = Kall @ qr[h] / np.sqrt(D)
                scores[(b, h)] = sc
                e = np.where(keep, np.exp(sc - sc[keep].max()), 0.0)
                out[b, h] = (e @ Vall) / (e.sum() + 1e-6)
    return out, scores


def decode_gaps(c, scores):
    """-> {(b, h): gap in nats of the largest planted key over every other key (history + new token)}."""
    gaps = {}
    tl = c["L"] - 1
    for (b, h), sc in scores.items():
        hk = h // (c["H"] // c["Hkv"])
        pl = [pos for (pb, ph, pos) in c["planted"] if pb == b and ph == hk]
        if not pl:
            continue
        isp = np.zeros(tl + 1, bool); isp[pl] = True
        gaps[(b, h)] = sc[:tl + 1][isp].max() - sc[:tl + 1][~isp].max()
    return gaps


# ---------------------------------------------------------------------------------------------------------------------
# the cases: one registry for the CPU checks and the GPU runs
# ---------------------------------------------------------------------------------------------------------------------
PREFILL_BAR = 2e-3                 # tests/test_flash_gpu.py TOL
DECODE_BAR = 1e-3                  # tests/test_attention_gpu.py TOL
SENS = 50                          # a probe must move the affected outputs by >= SENS x the bar
NEEDLES = [0, 1, 31, 32, 63, 64, 65, 127, 128, 129, 199]     # wave (32), key tile (64), workgroup (128) boundaries; last key
NEEDLES_BR = [150, 151, 160, 191, 192, 199]                   # lq = 50 < lk = 200: row i sees keys <= i + 150
GQA = {1: (2, 2), 4: (8, 2), 8: (8, 1)}
RAMPS = [0.5, 7.9, 8.1, 40.0]
SINKS = [4.0, 12.0, 30.0]


def _rows_of(c, b, sel):
    m = np.zeros(int(c["cu_q"][-1]), bool)
    m[int(c["cu_q"][b]) + np.asarray(sel, int)] = True
    return m


def prefill_spec(name):
    """-> dict(c, causal, probes=[(drop, admit, affected row mask [Tq])], top=None | (affected rows, min fraction),
    rows=None | {b: sampled rows}, zero_rows=row mask that must be exactly 0, packed=bool)."""
    kind, *a = name.split(":")
    if kind == "needle":                                   # needle:G:eq|br
        G, br = int(a[0]), a[1] == "br"
        H, Hkv = GQA[G]
        ns = NEEDLES_BR if br else NEEDLES
        lq = 50 if br else 200
        c = prefill_case([lq] * len(ns), [200] * len(ns), H, Hkv, {(b, n): 25.0 for b, n in enumerate(ns)}, seed=10 + G)
        sh = 200 - lq
        probes = []
        for b, n in enumerate(ns):
            probes.append(([(b, n)], [], _rows_of(c, b, range(max(0, n - sh), lq))))
            if n - sh - 1 >= 0:
                probes.append(([], [(b, int(c["cu_k"][b]) + n, "diag")], _rows_of(c, b, [n - sh - 1])))
        return dict(c=c, causal=True, probes=probes, packed=not br)
    if kind == "sink":                                     # sink:g:causal|full[:scale]
        g, causal = float(a[0]), a[1] == "causal"
        scale = float(a[2]) if len(a) > 2 else None
        lens = [300, 129, 1, 64]
        pl = {}
        for b, lk in enumerate(lens):
            pl[(b, 0)] = g + 6.0
            for j in (5, lk // 2, lk - 1):
                if 0 < j < lk:
                    pl[(b, j)] = 6.0
        c = prefill_case(lens, lens, 8, 2, pl, seed=int(g) + 3 * causal, scale=scale)
        return dict(c=c, causal=causal, packed=True,
                    probes=[([(b, 0)], [], _rows_of(c, b, range(lk))) for b, lk in enumerate(lens)])
    if kind == "ramp":                                     # ramp:r:causal|full
        rr, causal = float(a[0]), a[1] == "causal"
        c = ramp_case(1024, 4, 1, rr, seed=int(10 * rr))
        first = min(j for (_, j) in c["planted"])
        return dict(c=c, causal=causal, packed=True, probes=[], top=(_rows_of(c, 0, range(first, 1024)), 0.75))
    if kind == "late":                                     # late needle in one 8 192-key row, sampled rows
        c = prefill_case([8192], [8192], 8, 2, {(0, 8150): 20.0}, seed=81)
        rows = [0, 1, 63, 64, 4095, 8127, 8128, 8149, 8150, 8151, 8191]
        ri = np.arange(len(rows))
        return dict(c=c, causal=True, packed=True, rows={0: np.array(rows)},
                    probes=[([(0, 8150)], [], ri >= rows.index(8150)), ([], [(0, 8150, "diag")], ri == rows.index(8149))])
    if kind == "peaked":                                   # peaked:sigma:causal|full
        sigma, causal = float(a[0]), a[1] == "causal"
        lens = [1, 63, 200, 129]
        c = peaked_prefill_case(lens, lens, 8, 2, sigma, seed=int(sigma) + 7 * causal)
        return dict(c=c, causal=causal, packed=True, probes=[], top=(np.ones(int(c["cu_q"][-1]), bool), 0.5))
    if kind == "varlen":                                   # varlen:causal|full - neighbours and zero-length sequences
        causal = a[0] == "causal"
        lens = [100, 0, 100, 100, 0, 100]
        c = prefill_case(lens, lens, 8, 2, {(2, 0): 25.0, (3, 99): 25.0}, seed=5 + causal)
        ck = c["cu_k"]
        return dict(c=c, causal=causal, packed=True,
                    probes=[([], [(0, int(ck[2]), "after")], _rows_of(c, 0, [99] if causal else range(100))),
                            ([], [(5, int(ck[3]) + 99, "before")], _rows_of(c, 5, range(100))),
                            ([(2, 0)], [], _rows_of(c, 2, range(100))), ([(3, 99)], [], _rows_of(c, 3, [99] if causal else range(100)))])
    if kind == "empty":                                    # empty:causal|full - rows without a visible key: exactly 0
        causal = a[0] == "causal"
        lq, lk = [100, 70, 10], [40, 70, 0]
        c = prefill_case(lq, lk, 8, 2, {(0, 0): 25.0}, seed=9 + causal)
        zero = np.zeros(180, bool)
        zero[170:] = True
        if causal:
            zero[:60] = True
        probes = [([], [(0, int(c["cu_k"][0]), "diag")], _rows_of(c, 0, [59]))] if causal else \
                 [([(0, 0)], [], _rows_of(c, 0, range(100)))]
        return dict(c=c, causal=causal, packed=False, probes=probes, zero_rows=zero)
    raise KeyError(name)


PREFILL_CASES = ([f"needle:{g}:{m}" for g in GQA for m in ("eq", "br")] +
                 [f"sink:{g:g}:{m}" for g in SINKS for m in ("causal", "full")] + ["sink:12:full:0.05", "sink:4:causal:0.2"] +
                 [f"ramp:{r:g}:{m}" for r in RAMPS for m in ("causal", "full")] + ["late"] +
                 [f"peaked:{s}:{m}" for s in (4, 8) for m in ("causal", "full")] +
                 [f"varlen:{m}" for m in ("causal", "full")] + [f"empty:{m}" for m in ("causal", "full")])


def decode_spec(name):
    """-> dict(c, probes=[(drop, admit, affected {(b, h)})], top=None | min fraction)."""
    kind, *a = name.split(":")
    int4 = a[0] == "kv4"
    if kind == "needle":                                   # needle:kv:G - every split boundary of the plans tested
        G = int(a[1])
        L, Hkv = 1033, 2
        pos = {0, 31, 32, 63, 64, L - 2, L - 1}
        for n in (1, 2, 3, 4, 7, 8, 16):                    # forced splits and what the planner picks here
            pos |= set(split_boundaries(L, n, int4))
        pos = sorted(pos)
        B = max(32, len(pos))
        pl = {(b, hk, pos[(b + 7 * hk) % len(pos)]): 25.0 for b in range(B) for hk in range(Hkv)}
        c = decode_case(B, Hkv * G, Hkv, L, int4, pl, seed=100 + G + 10 * int4)
    elif kind == "sink":                                   # sink:kv:L
        L = int(a[1])
        pl = {}
        for b, g in enumerate(SINKS):
            for hk in range(2):
                pl[(b, hk, 0)] = g + 6.0
                for j in (L // 3, L - 2, L - 1)[hk:]:
                    pl[(b, hk, j)] = 6.0
        c = decode_case(len(SINKS), 8, 2, L, int4, pl, seed=L + int4)
    elif kind == "onesplit":                               # onesplit:kv:gap - the maximum in one split of 7, the rest trail
        gap = float(a[1])
        L = 1033
        firsts = split_boundaries(L, 7, int4)
        tops = [(firsts[2 * z] + firsts[2 * z + 1]) // 2 for z in range(len(firsts) // 2)] + [firsts[1], firsts[-2]]
        pl = {(b, hk, tops[(b + 3 * hk) % len(tops)]): gap + 3.0 for b in range(len(tops)) for hk in range(2)}
        c = decode_case(len(tops), 8, 2, L, int4, pl, seed=int(gap) + int4, s=4.0)
    elif kind == "newtok":                                 # newtok:kv:G - the new token +20 nats / 30 nats under the max
        G, L = int(a[1]), 1033
        pl = {}
        for hk in range(2):
            pl[(0, hk, L - 1)] = 20.0
            pl[(1, hk, L - 1)] = 20.0
            pl[(2, hk, 500 + hk)] = 20.0
            pl[(2, hk, L - 1)] = -10.0
            pl[(3, hk, L - 2)] = 20.0
            pl[(3, hk, L - 1)] = -10.0
        c = decode_case(4, 2 * G, 2, L, int4, pl, seed=7 + G + int4)
        probes = [([(b, hk, p)], [], {(b, h) for h in range(hk * G, hk * G + G)}) for (b, hk, p), lv in pl.items() if lv > 0]
        return dict(c=c, probes=probes)
    elif kind == "peaked":                                 # peaked:kv:sigma
        c = decode_case(4, 8, 2, 1033, int4, {}, seed=int(a[1]) + int4, sigma_q=float(a[1]))
        return dict(c=c, probes=[], top=0.5)
    elif kind == "anti":                                   # anti:kv - finite huge keys past the sequence end
        L = 1033
        slots = [1033, 1055, 1056, 1087]
        anti = [(b, hk, slots[(b + hk) % 4], 40.0) for b in range(4) for hk in range(2)]
        c = decode_case(4, 8, 2, L, int4, {}, seed=3 + int4, anti=anti)
        return dict(c=c, probes=[([], [(b, hk, sl)], {(b, h) for h in range(4 * hk, 4 * hk + 4)}) for (b, hk, sl, _) in anti])
    else:
        raise KeyError(name)
    G = c["H"] // c["Hkv"]
    probes = [([(b, hk, p)], [], {(b, h) for h in range(hk * G, hk * G + G)}) for (b, hk, p) in c["planted"]
              if c["planted"][(b, hk, p)] > 6.0]
    return dict(c=c, probes=probes)


DECODE_CASES = ([f"needle:{kv}:{g}" for kv in ("kv4", "kv8") for g in (1, 4, 5, 8)] +
                [f"sink:{kv}:1033" for kv in ("kv4", "kv8")] + ["sink:kv8:8191"] +
                [f"onesplit:{kv}:{g}" for kv in ("kv4", "kv8") for g in (30, 100)] +
                [f"newtok:{kv}:{g}" for kv in ("kv4", "kv8") for g in (4, 5)] +
                [f"peaked:{kv}:{s}" for kv in ("kv4", "kv8") for s in (4, 8)] + [f"anti:{kv}" for kv in ("kv4", "kv8")])


@functools.lru_cache(maxsize=None)
def prefill(name):
    """The case with its float64 reference (token layout; sampled rows for "late"), cached per process."""
    sp = prefill_spec(name)
    sp["ref"] = prefill_ref(sp["c"], sp["causal"], rows=sp.get("rows"))
    return sp


@functools.lru_cache(maxsize=None)
def decode(name):
    """The case with kvattn.decode_attention(mode="exact") and the pool after the step, cached per process."""
    sp = decode_spec(name)
    sp["ref"], sp["pool_after"] = oracle_decode(sp["c"])
    return sp



def dequant_rounding_bound(c):
    """First-order bound [B, H, D] on |attention over the fp16 de-quantised cache - attention over the exact one|, from the
    VALU kernel's stated roundings (attention.hip: K and V de-quantised to fp16 as the reference does - KV4
    hfma2(n, fp16(scale), fp16(-scale * zero)), KV8 fp16(scale * (n - zero)) - scores, softmax and P.V in fp32).
    Per cached element the fp16 value is off by at most e = ulp(value) / 2, plus ulp(fp16(-scale * zero)) / 2 for KV4.
    A token's score then moves by ds_j <= sum_d |q_d| e_jd / sqrt(128), and with dO/ds_j = p_j (v_j - O) the output by
        sum_j p_j (|v_jd - O_d| ds_j + e^V_jd),
    times exp(2 max ds) for the second-order terms (the exponential and the normalisation).  The new token's k and v are
    used unrounded (no term).  At |q| ~ 8 sqrt(128) (peaked random, sigma_q = 8) this reaches several 1e-3: the rounding
    of a cache value of ~3 is 2^-10, and it is multiplied by |q|_1 / sqrt(128) ~ 64."""
    pool, int4 = c["pool"], c["int4"]
    B, H, _ = c["q"].shape
    Hkv = c["Hkv"]
    G = H // Hkv
    bound = np.zeros((B, H, D))
    ex, scores = decode_exact(c)

    def half_ulp(x):
        return np.spacing(np.abs(np.asarray(x, np.float16))).astype(np.float64) / 2

    for b in range(B):
        tl = int(c["lengths"][b]) - 1
        qr = kvattn.rope_neox(c["q"][b], tl, ROPE).astype(np.float64)
        for hk in range(Hkv):
            errs = []
            for which, col in (("k", 0), ("v", 1)):
                qb, sc, zr = pool.read_tokens(which, c["tables"][b, col], hk, tl)
                e = half_ulp(kvattn.kv_dequantize(qb, sc, zr, int4, "kernel"))
                if int4:
                    hz = (-(sc.astype(np.float32)) * zr.astype(np.float32)).astype(np.float32)
                    e = e + half_ulp(hz)[:, None]
                errs.append(np.concatenate([e, np.zeros((1, D))]))          # the new token: no rounding
            eK, eV = errs
            Vd = np.concatenate([kvattn.kv_dequantize(*pool.read_tokens("v", c["tables"][b, 1], hk, tl), int4, "exact"),
                                 c["v"][b, hk][None].astype(np.float32)]).astype(np.float64)
            for g in range(G):
                h = hk * G + g
                s = scores[(b, h)][:tl + 1]
                p = np.exp(s - s.max()); p /= p.sum()
                ds = eK @ np.abs(qr[h]) / np.sqrt(D)
                bound[b, h] = (p[:, None] * (np.abs(Vd - ex[b, h][None]) * ds[:, None] + eV)).sum(axis=0) * np.exp(2 * ds.max())
    return bound


@functools.lru_cache(maxsize=None)
def decode_fp16_cache(name):
    """Attention over the fp16 de-quantised cache the VALU kernel computes (kv_dequantize mode "kernel"), float64 math."""
    return decode_exact(decode(name)["c"], deq="kernel")[0]


@functools.lru_cache(maxsize=None)
def decode_rounding_bound(name):
    return dequant_rounding_bound(decode(name)["c"])
