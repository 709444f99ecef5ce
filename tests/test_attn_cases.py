"""CPU half of the peaked-softmax attention tests (tests/_attn_cases.py, run on the GPU by tests/test_attn_peaked_gpu.py): the
builders reach the score gaps they are designed for, the restated references equal the oracles, every probe (a planted key
dropped, a masked key admitted) moves the affected outputs by >= 50x the GPU bar, and the per-tile ramps cause the number of
lazy-maximum rescales they are meant to."""
import numpy as np
import pytest

import _attn_cases as A
from oracle import flash as oflash
from oracle import kvattn


def test_rope_inverse_round_trip():
    r = np.random.default_rng(0)
    x = (4 * r.standard_normal((5, 128))).astype(np.float16)
    for pos in (0, 1, 1032, 8190):
        y = kvattn.rope_neox(kvattn.rope_neox_inv(x, pos, A.ROPE), pos, A.ROPE).astype(np.float32)
        assert np.abs(y - x.astype(np.float32)).max() <= 2 * np.spacing(np.float16(16)), pos


def test_split_boundaries():
    assert A.split_boundaries(1033, 7, True) == [0, 159, 160, 319, 320, 479, 480, 639, 640, 799, 800, 959, 960, 1031]
    assert A.split_boundaries(1033, 2, False) == [0, 575, 576, 1031]
    assert A.split_boundaries(70, 7, True) == [0, 31, 32, 63, 64, 68]     # 3 units: the last splits are empty


@pytest.mark.parametrize("name", A.PREFILL_CASES)
def test_prefill_case(name):
    sp = A.prefill(name)
    c, causal, bar = sp["c"], sp["causal"], A.PREFILL_BAR
    rows = sp.get("rows")
    # the restated reference is the oracle's definition
    if rows is None:
        ref = A.to_tokens(c, sp["ref"])
        assert np.abs(ref - A.oracle_prefill(c, causal)).max() < 1e-6
        assert (np.abs(ref).max() < 1.0) and np.isfinite(ref).all()
    else:
        rr = rows[0] + int(c["cu_q"][0])
        ora = oflash.attention_rows(c["q"], c["k"], c["v"], c["cu_q"], c["cu_k"], list(rr), list(range(c["H"])),
                                    scale=c["scale"], causal=causal)
        ref = sp["ref"][0].transpose(1, 0, 2)
        assert np.abs(ref - ora).max() < 1e-6
    if "zero_rows" in sp:
        assert sp["zero_rows"].any() and (ref[sp["zero_rows"]] == 0).all()
    # reached gaps
    kind = name.split(":")[0]
    gaps = A.reached_gaps(c, causal, rows=rows)
    if kind in ("needle", "varlen", "late", "empty"):
        lev = min(c["planted"].values())
        for g in gaps.values():
            seen = np.isfinite(g)
            assert seen.any() and (g[seen] > lev - 2.0).all(), (lev, np.nanmin(g))
    if kind == "sink":
        gsink = float(name.split(":")[1])
        for b in range(len(c["cu_q"]) - 1):
            S, vis, _ = A._seq_scores(c, b, None, causal)
            if S.shape[2] < 2:
                continue
            g = S[:, :, 0] - np.where(vis[None, :, 1:], S[:, :, 1:], -np.inf).max(axis=2)
            seen = vis[:, 1:].any(axis=1)
            assert (g[:, seen] > gsink - 0.5).all()                 # key 0 leads every other key by g
            assert np.abs(g[:, 6:] - gsink).max() < 0.5             # ... and by exactly g once a runner-up (key 5) is visible
    # sensitivity: every probe moves every head of every affected row by >= 50x the bar
    for drop, admit, affected in sp["probes"]:
        only = {d[0] for d in drop} | {a[0] for a in admit}
        alt = A.prefill_ref(c, causal, rows=rows, drop=drop, admit=admit, only=only)
        alt = A.to_tokens(c, alt) if rows is None else alt[0].transpose(1, 0, 2)
        moved = np.abs(alt - ref).max(axis=2)                       # [rows, H]
        assert affected.any() and moved[affected].min() >= A.SENS * bar, (drop, admit, moved[affected].min())
    if sp.get("top") is not None:
        affected, frac = sp["top"]
        moved = A.top_key_change(c, causal)[affected]
        assert (moved >= A.SENS * bar).mean() >= frac, (moved >= A.SENS * bar).mean()


@pytest.mark.parametrize("r", A.RAMPS)
def test_ramp_rescale_counts(r):
    """The round-6 kernel's lazy maximum on the reached scores of the ramps, for the rows that see all 16 tiles: r = 0.5 never
    moves it (probabilities up to 2^7.5); r = 7.9 moves it on every second tile and lets probabilities reach 2^7.9 in
    between; r = 8.1 and 40 move it on every tile, the latter scaling the old O by 2^-40."""
    c = A.prefill(f"ramp:{r:g}:full")["c"]
    cnt, pmax, amin = A.lazy_rescales(c, causal=False)
    # the design's closed form
    m, want, wp = 4.0, 0, 1.0
    for t in range(1, 16):
        mx = 4.0 + r * t
        if mx > m + A.LAZY:
            want, m = want + 1, mx
        wp = max(wp, 2.0 ** (mx - m))
    assert (cnt == want).all(), (np.unique(cnt), want)
    assert want == {0.5: 0, 7.9: 7, 8.1: 15, 40.0: 15}[r]
    assert np.abs(np.log2(pmax) - np.log2(wp)).max() < 0.2
    if r >= 8:      # (the planted keys' fp16 rounding, 2^-12 relative, is ~0.3 log2 units at the r = 40 ramp's ~600)
        assert np.abs(np.log2(amin) + r).max() < 0.5
    cc, _, _ = A.lazy_rescales(c, causal=True)
    assert cc.max() == want and cc.min() == 0                     # causal: the rows of the first tiles see fewer tiles


@pytest.mark.parametrize("name", A.DECODE_CASES)
def test_decode_case(name):
    sp = A.decode(name)
    c, ref, bar = sp["c"], sp["ref"], A.DECODE_BAR
    ex, scores = A.decode_exact(c)
    assert np.abs(ex - ref.astype(np.float64)).max() <= 2.5e-4        # the restatement = the oracle up to its fp16 output
    assert np.isfinite(ref).all() and np.abs(ref).max() < 1.0
    kind = name.split(":")[0]
    gaps = A.decode_gaps(c, scores)
    tl = c["L"] - 1
    if kind == "needle":
        assert len(gaps) == c["q"].shape[0] * c["H"] and min(gaps.values()) > 23.0, min(gaps.values())
    if kind == "sink":
        for (b, h), sc in scores.items():
            assert abs(sc[0] - sc[1:tl + 1].max() - A.SINKS[b]) < 0.5
    if kind == "onesplit":
        # the maximum lives in one split of 7: every other split's maximum trails it by >= the gap - 2 nats
        sb = A.split_boundaries(c["L"], 7, c["int4"])
        for (b, h), sc in scores.items():
            top = int(np.argmax(sc[:tl + 1]))
            for z in range(len(sb) // 2):
                if not sb[2 * z] <= top <= sb[2 * z + 1]:
                    assert sc[top] - sc[sb[2 * z]:sb[2 * z + 1] + 1].max() > float(name.split(":")[2])
            assert sc[top] - sc[tl] > float(name.split(":")[2])             # and so does the new token
    if kind == "newtok":
        for (b, h), sc in scores.items():
            new_gap = sc[tl] - np.delete(sc[:tl + 1], tl).max()
            assert (new_gap > 18.0) if b < 2 else (new_gap < -28.0), (b, h, new_gap)
    if kind == "anti":
        for (b, hk, slot, _) in c["anti"]:
            _, sc2 = A.decode_exact(c, admit=[(b, hk, slot)], only={b})
            G = c["H"] // c["Hkv"]
            assert sc2[(b, hk * G)][-1] - sc2[(b, hk * G)][:tl + 1].max() > 30.0   # it would dominate if it leaked
    for drop, admit, affected in sp["probes"]:
        alt, _ = A.decode_exact(c, drop=drop, admit=admit, only={b for (b, _) in affected})
        moved = np.array([np.abs(alt[b, h] - ex[b, h]).max() for (b, h) in affected])
        assert moved.min() >= A.SENS * bar, (drop, admit, moved.min())
    if sp.get("top") is not None:
        moved = []
        for (b, h), sc in scores.items():
            hk = h // (c["H"] // c["Hkv"])
            alt, _ = A.decode_exact(c, drop=[(b, hk, int(np.argmax(sc)))], only={b})
            moved.append(np.abs(alt[b, h] - ex[b, h]).max())
        assert (np.array(moved) >= A.SENS * bar).mean() >= sp["top"], moved


@pytest.mark.parametrize("name", [n for n in A.DECODE_CASES if n.startswith("peaked")])
def test_dequant_rounding_bound_covers_the_fp16_cache(name):
    """The VALU kernel de-quantises the cache to fp16 (the reference's form).  On peaked random scores that rounding alone
    moves the output by up to ~6e-3 (KV4, sigma_q = 8): the derived bound must cover it, element by element, and the
    fp16-cache attention must sit that far from the exact one (what the GPU test's two references separate)."""
    c = A.decode(name)["c"]
    ex, _ = A.decode_exact(c)
    f16 = A.decode_fp16_cache(name)
    bound = A.decode_rounding_bound(name)
    assert (np.abs(f16 - ex) <= bound).all()
    if name == "peaked:kv4:8":
        assert np.abs(f16 - ex).max() > 2 * A.DECODE_BAR
