"""The sliding-window decode and append entries (csrc/attention_window.hip, csrc/append_window.hip) against float64 attention over the
de-quantised pool with the mask p - W < j <= p, at LC.TOL: finite, pools bit-equal to the unchanged writer's, a second run bit-identical.
For W in {64, 65, 130} the last key below the window and the window's first key are planted, so that an off-by-one moves the result
far beyond the bar; both conditions are asserted on the host."""
import functools

import numpy as np
import pytest
import torch

import _attn_cases as AC
import _long_cases as LC
import _rope_scaling_cases as RC
from _append_cases import compose, host_pool, rotate_rows, scattered_tables
from _helpers import DevPools, dev
from oracle import kvattn

pytestmark = pytest.mark.gpu
KV = [pytest.param(True, id="kv4"), pytest.param(False, id="kv8")]
HEADS = [(8, 2), (5, 1)]
TOL, MB = LC.TOL, 16
DECODE_PASTS = [0, 63, 64, 200, 700]
APPEND = [(0, 200, 64), (130, 5, 64), (700, 40, 130), (63, 2, 1), (200, 70, 10000)]
PLANTED = (64, 65, 130)


def windowed(q, K, V, cu_q, cu_k, past, W, admit=(), drop=()):
    """float64 [T, H, 128]: row i of sequence b, at p = past[b] + i, sees key j iff p - W < j <= p; admit / drop: (b, j) keys let in / out."""
    H, G = q.shape[1], q.shape[1] // K.shape[1]
    out = np.zeros(q.shape, np.float64)
    for b in range(len(past)):
        qs, ks, n, L = int(cu_q[b]), int(cu_k[b]), int(cu_q[b + 1] - cu_q[b]), int(cu_k[b + 1] - cu_k[b])
        p, j = int(past[b]) + np.arange(n)[:, None], np.arange(L)[None, :]
        vis = (j > p - W) & (j <= p)
        vis[:, [jj for bb, jj in admit if bb == b]] = True
        vis[:, [jj for bb, jj in drop if bb == b]] = False
        for h in range(H):
            S = q[qs:qs + n, h].astype(np.float64) @ K[ks:ks + L, h // G].astype(np.float64).T / np.sqrt(128.0)
            P = np.exp(np.where(vis, S, -np.inf) - np.where(vis, S, -np.inf).max(axis=1, keepdims=True))
            out[qs:qs + n, h] = (P / P.sum(axis=1, keepdims=True)) @ V[ks:ks + L, h // G].astype(np.float64)
    return out


@functools.lru_cache(maxsize=None)
def problem(H, Hkv, int4, pasts, ns, W):
    """pasts[b] cached and ns[b] new tokens under scattered tables: host pool, rows, and - once - reference, expected pools, conditions."""
    from qserve_amd import rope
    prof = (rope.base_denominators(RC.BASE), np.float32(1.0))
    r = np.random.default_rng(5 + 8 * H + Hkv + int(int4) + 3 * W + sum(pasts))
    G, B, past = H // Hkv, len(pasts), np.asarray(pasts, np.int32)
    cu = np.concatenate([[0], np.cumsum(ns)]).astype(np.int32)
    tables, nblocks = scattered_tables(r, B, MB)
    host0 = kvattn.PagePool(nblocks, Hkv, 128, int4, fill=0xFF)
    RC.history(host0, r, tables, pasts, H, Hkv, prof)
    new = r.standard_normal((int(cu[-1]), (H + 2 * Hkv) * 128)).astype(np.float16)
    planted = []        # (sequence, row, key below the window, the window's first key): both planted, seen from the sequence's last row
    if W in PLANTED:
        qrot = RC.rotate_rows(new, cu, past, H, Hkv, prof)
        for b in range(B):
            row, p = int(cu[b + 1]) - 1, int(past[b]) + ns[b] - 1
            if p - W < 0:
                continue
            planted.append((b, row, p - W, p - W + 1))
            for j, sign in ((p - W, -1.0), (p - W + 1, 1.0)):      # k = the row's rotated query (first head of the group), v = -+ a pattern
                kr = qrot[row, :H * 128].reshape(Hkv, G, 128)[:, 0]
                vv = np.tile(0.75 * sign * np.where(np.arange(128) % 2, -1.0, 1.0), (Hkv, 1)).astype(np.float16)
                if j < past[b]:
                    (kb, ks, kz), (vb, vs, vz) = kvattn.kv_quantize(kr, int4), kvattn.kv_quantize(vv, int4)
                    for h in range(Hkv):
                        host0.write_token("k", int(tables[b, 0, j // 64]), j % 64, h, kb[h], ks[h], kz[h])
                        host0.write_token("v", int(tables[b, 1, j // 64]), j % 64, h, vb[h], vs[h], vz[h])
                else:                                              # a new key: its un-rotated row
                    t = int(cu[b]) + j - int(past[b])
                    new[t, H * 128:(H + Hkv) * 128] = kvattn.rope_neox_inv(kr, j, RC.BASE).reshape(-1)
                    new[t, (H + Hkv) * 128:] = vv.reshape(-1)
    rot, want_k, want_v = RC.expect_writer(host0, new, cu, past, tables, H, Hkv, prof)
    q, K, V, cu_k = compose(rot, cu, past, tables, host0, H, Hkv)
    ref = windowed(q, K, V, cu, cu_k, past, W)
    for b, row, below, first in planted:
        heads = np.arange(Hkv) * G
        leak = np.abs(windowed(q, K, V, cu, cu_k, past, W, admit=[(b, below)]) - ref)[row, heads].max(axis=1).min()
        lost = np.abs(windowed(q, K, V, cu, cu_k, past, W, drop=[(b, first)]) - ref)[row, heads].max(axis=1).min()
        print(f"WINDOW planted seq {b} W={W}: admitting key {below} moves >= {leak:.3f}, dropping key {first} >= {lost:.3f}")
        assert leak >= AC.SENS * TOL and lost >= AC.SENS * TOL, (b, leak, lost)
    assert planted or W not in PLANTED or max(p + n for p, n in zip(pasts, ns)) <= W, "no sequence long enough to plant in"
    return dict(tables=tables, nblocks=nblocks, host0=host0, new=new, cu=cu, past=past, ref=ref.astype(np.float32), want_k=want_k, want_v=want_v)


def decode(new, kvp, lengths, H, Hkv, int4, base, timestep, W, splits=0):
    from qserve_amd.long_decode import single_query_attention_long
    q, k, v = [x.reshape(new.size(0), -1, 128) for x in new.split([H * 128, Hkv * 128, Hkv * 128], dim=-1)]
    return single_query_attention_long(q, k, v, kvp, lengths, Hkv * (64 if int4 else 128), timestep, base, int4, num_splits=splits, window=W)


def run(c, H, Hkv, int4, W, decode_splits=None):
    from qserve_amd import append
    pools = DevPools(c["nblocks"], Hkv, int4, "cuda:0")
    pools.k.copy_(dev(c["host0"].k)), pools.v.copy_(dev(c["host0"].v))
    new, kvp, spt = dev(c["new"]), pools.pointers(c["tables"]), Hkv * (64 if int4 else 128)
    if decode_splits is None:
        out = append.append(new, dev(c["cu"]), dev(c["past"]), kvp, H, Hkv, spt, RC.BASE, int4, max_seqlen_q=int(np.diff(c["cu"]).max()), window=W)
    else:
        out = decode(new, kvp, dev(c["past"] + 1), H, Hkv, int4, RC.BASE, MB * 64, W, decode_splits)
    torch.cuda.synchronize()
    return out.cpu().numpy(), pools.k.cpu().numpy(), pools.v.cpu().numpy()


def check(c, H, Hkv, int4, W, what, decode_splits=None):
    out, k, v = run(c, H, Hkv, int4, W, decode_splits)
    err = float(np.abs(out.astype(np.float32) - c["ref"].reshape(out.shape)).max())
    print(f"WINDOW {what} H={H} Hkv={Hkv} int4={int4} W={W} splits={decode_splits}: max abs err {err:.3e}")
    assert np.isfinite(out.astype(np.float32)).all() and err <= TOL, f"max abs err {err:.2e}"
    assert np.array_equal(k, c["want_k"]) and np.array_equal(v, c["want_v"]), "pages: the writer's bytes changed"
    assert all(np.array_equal(a, b) for a, b in zip((out, k, v), run(c, H, Hkv, int4, W, decode_splits))), "a second run differs"


@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("W", [1, 64, 65, 130, 10000])
@pytest.mark.parametrize("H,Hkv", HEADS)
@pytest.mark.parametrize("int4", KV)
def test_decode_window(gpu, int4, H, Hkv, W, splits):
    check(problem(H, Hkv, int4, tuple(DECODE_PASTS), (1,) * len(DECODE_PASTS), W), H, Hkv, int4, W, "decode", splits)


@pytest.mark.parametrize("past,n,W", APPEND)
@pytest.mark.parametrize("H,Hkv", HEADS)
@pytest.mark.parametrize("int4", KV)
def test_append_window(gpu, int4, H, Hkv, past, n, W):
    check(problem(H, Hkv, int4, (past, past + 70), (n, max(1, n // 2)), W), H, Hkv, int4, W, "append, two sequences of different past")


@pytest.mark.parametrize("int4", KV)
def test_decode_window_past_the_address_staging(gpu, int4):
    """A 260-entry table (more than the 256 addresses staged at a time), past 16 500, W = 4 096; the planner's ranges and one range."""
    from qserve_backend import fused_attention as fa
    W, case = 4096, LC.Case(8, 2, int4, [16500], [1], 260, 91 + int(int4))
    H, Hkv, n = case.H, case.Hkv, case.hist_len
    pools = DevPools(case.nblocks, Hkv, int4, "cuda:0")
    fa.apply_bias_rope_update_kv_cache(dev(case.hist), dev(np.asarray([n], np.int32)),
                                       fa.compute_padding_offsets(dev(np.asarray([0, n], np.int32)), n, n), pools.pointers(case.hist_tables),
                                       H, Hkv, n, 64, case.spt, 128, LC.BASE, 8192, True, int4, True)
    torch.cuda.synchronize()
    hp = host_pool(pools.k.cpu().numpy(), pools.v.cpu().numpy(), Hkv, int4)
    rot = rotate_rows(case.new, case.cu_q, case.past, H, Hkv, LC.BASE)
    q, K, V, cu_k = compose(rot, case.cu_q, case.past, case.tables, hp, H, Hkv)
    ref = windowed(q, K, V, case.cu_q, cu_k, case.past, W)
    moved = float(np.abs(windowed(q, K, V, case.cu_q, cu_k, case.past, 2 * W) - ref).max(axis=2).min())
    assert moved >= 5 * TOL, f"a window twice as long moves the reference by only {moved:.4f}"
    RC.write_rows(hp, case.new, rot, case.cu_q, case.past, case.tables, H, Hkv)
    before = pools.k.clone(), pools.v.clone()
    for splits in (0, 1):
        pools.k.copy_(before[0]), pools.v.copy_(before[1])
        out = decode(dev(case.new), pools.pointers(case.tables), dev(case.past + 1), H, Hkv, int4, LC.BASE, 260 * 64, W, splits)
        torch.cuda.synchronize()
        err = float(np.abs(out.cpu().numpy().astype(np.float32) - ref.reshape(1, H, 128)).max())
        assert np.isfinite(out.cpu().numpy().astype(np.float32)).all() and err <= TOL, f"splits={splits}: max abs err {err:.2e}"
        assert np.array_equal(pools.k.cpu().numpy(), hp.k) and np.array_equal(pools.v.cpu().numpy(), hp.v), "pages: the new token's slot, or a byte elsewhere"


@pytest.mark.parametrize("int4", KV)
def test_captured_decode_follows_the_window(gpu, int4):
    """W = 64 at pasts (126, 300) -> (128, 302): the first sequence's window start moves from page 0 (token 63) to page 1 (token 64).
    Three replays, the lengths advanced on the device between them, each bit-equal to an eager call at the same lengths."""
    H, Hkv, W = 8, 2, 64
    c = problem(H, Hkv, int4, (126, 300), (3, 3), 10000)      # (its rows serve as three steps' new tokens)
    gp, ep = DevPools(c["nblocks"], Hkv, int4, "cuda:0"), DevPools(c["nblocks"], Hkv, int4, "cuda:0")
    for p in (gp, ep):
        p.k.copy_(dev(c["host0"].k)), p.v.copy_(dev(c["host0"].v))
    rows = dev(c["new"]).view(2, 3, -1)
    new, lengths = rows[:, 0].clone(), dev(c["past"] + 1)
    kvp_g, kvp_e = gp.pointers(c["tables"]), ep.pointers(c["tables"])
    call = lambda kvp: decode(new, kvp, lengths, H, Hkv, int4, RC.BASE, MB * 64, W)      # noqa: E731
    call(kvp_g)                                               # outside the capture: the split-KV workspace's first use
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = call(kvp_g)
    for i in range(3):
        new.copy_(rows[:, i])
        g.replay()
        eager = call(kvp_e)
        torch.cuda.synchronize()
        assert torch.isfinite(out.float()).all() and torch.equal(out, eager), f"replay {i}: output differs from the eager call"
        assert torch.equal(gp.k, ep.k) and torch.equal(gp.v, ep.v), f"replay {i}: pages differ"
        lengths.add_(1)
