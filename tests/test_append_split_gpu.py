"""GPU parity of split-KV append attention (qs_append_attention_split; qserve_amd.append with max_past / num_splits): forced split
counts against the float64 composition of the existing oracles (tests/_append_cases.py) at the bar of tests/test_append_gpu.py,
stale workspace contents, one split = today's kernel bit for bit, the length hint as a mere hint, planted keys that single out one
split's weight in the merge, determinism, graph capture (with and without the workspace) and padded layouts."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _attn_cases as AC
from _append_cases import expected, host_pool, rotate_rows, scattered_tables
from _helpers import DevPools, dev

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 2e-3      # tests/test_append_gpu.py TOL: an fp16 MFMA attention against a float64 oracle on standard normal inputs
BASE = 1e4
KV = [pytest.param(True, id="kv4"), pytest.param(False, id="kv8")]
# ragged batch: 16 pages in the longest past (16 splits = one page each there, empty splits everywhere else), pasts around the page
# boundary, no past at all (phase 2 only), n = 0, n = 130 (several query tiles for G >= 2)
PASTS = [0, 1, 63, 64, 65, 200, 640, 1000]
NS = [5, 1, 8, 3, 0, 33, 4, 130]
SHORT_PASTS = [64, 65, 100, 128, 1, 127, 90, 70]      # 1 to 2 pages each: 14 to 15 of 16 splits empty


def _spt(Hkv, int4):
    return Hkv * (64 if int4 else 128)


def _np(t):
    return t.detach().cpu().numpy()


class _Canaried:
    """out [T, H, 128] fp16 between two 4 KiB areas of 0xA5."""

    def __init__(self, T, H, device):
        self.raw = torch.full((8192 + T * H * 256,), 0xA5, dtype=torch.uint8, device=device)
        self.out = self.raw[4096:4096 + T * H * 256].view(torch.float16).view(T, H, 128)

    def check(self):
        assert bool((self.raw[:4096] == 0xA5).all()) and bool((self.raw[-4096:] == 0xA5).all()), "write outside `out`"


def _spare_blocks_untouched(pools, tables, nblocks):
    used_k, used_v = set(tables[:, 0].ravel().tolist()), set(tables[:, 1].ravel().tolist())
    for name, pool, used in (("K", pools.k, used_k), ("V", pools.v, used_v)):
        spare = [i for i in range(nblocks) if i not in used]
        assert spare and bool((pool[spare] == 0xFF).all()), f"a {name} page of no sequence was written"


@functools.lru_cache(maxsize=None)
def _case(H, Hkv, int4, pasts, ns, seed):
    """The cache filled with `pasts` tokens (existing prefill writer), the append writer run on the new rows, the un-split attention
    and the oracle composition - once per configuration; the attention never writes a page, so every test re-uses them."""
    from qserve_amd import append as A
    from qserve_backend import fused_attention as fa
    gpu = torch.device("cuda:0")
    r = np.random.default_rng(seed)
    B, W = len(pasts), (H + 2 * Hkv) * 128
    mb = (max(p + n for p, n in zip(pasts, ns)) + 63) // 64 + 1
    tables, nblocks = scattered_tables(r, B, mb)
    pools = DevPools(nblocks, Hkv, int4, gpu)
    kvp = pools.pointers(tables)
    live = [b for b in range(B) if pasts[b] > 0]
    lens = [pasts[b] for b in live]
    ctx = dev(r.standard_normal((sum(lens), W)).astype(np.float16))
    cu_ctx = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    fa.apply_bias_rope_update_kv_cache(ctx, dev(np.asarray(lens, np.int32)), fa.compute_padding_offsets(dev(cu_ctx), max(lens), sum(lens)),
                                       pools.pointers(tables[live]), H, Hkv, max(lens), 64, _spt(Hkv, int4), 128, BASE, 8192, True, int4,
                                       True)
    T = int(sum(ns))
    src = r.standard_normal((T, W)).astype(np.float16)
    cu_q = np.concatenate([[0], np.cumsum(ns)]).astype(np.int32)
    past = np.asarray(pasts, np.int32)
    qkv = dev(src)
    A.append_rope_update_kv_cache(qkv, dev(cu_q), dev(past), kvp, H, Hkv, _spt(Hkv, int4), BASE, int4)
    unsplit = A.append_attention(qkv, dev(cu_q), dev(past), kvp, H, Hkv, _spt(Hkv, int4), int4, max_seqlen_q=int(max(ns)))
    torch.cuda.synchronize()
    hp = host_pool(_np(pools.k), _np(pools.v), Hkv, int4)
    ref = expected(_np(qkv), cu_q, past, tables, hp, H, Hkv)
    return dict(H=H, Hkv=Hkv, int4=int4, spt=_spt(Hkv, int4), B=B, T=T, W=W, mb=mb, msq=int(max(ns)), src=dev(src), qkv=qkv, cu_q=dev(cu_q),
                past=dev(past), kvp=kvp, pools=pools, pages=(pools.k.clone(), pools.v.clone()), tables=tables, nblocks=nblocks,
                unsplit=unsplit, ref=ref)


def _attend(c, out=None, **kw):
    from qserve_amd import append as A
    return A.append_attention(c["qkv"], c["cu_q"], c["past"], c["kvp"], c["H"], c["Hkv"], c["spt"], c["int4"], max_seqlen_q=c["msq"],
                              out=out, **kw)


def _err(c, out, what):
    got = _np(out).astype(np.float32)
    assert np.isfinite(got).all(), f"{what}: non-finite output"
    err = float(np.abs(got - c["ref"]).max())
    print(f"{what}: max abs err {err:.3e}")
    return err


def _ragged(H, Hkv, int4):
    return _case(H, Hkv, int4, tuple(PASTS), tuple(NS), 11 * H + Hkv + int(int4))


# ---- 1. forced splits against the oracle ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("splits", [2, 3, 7, 16])
@pytest.mark.parametrize("int4", KV)
@pytest.mark.parametrize("H,Hkv", [(8, 2), (4, 4), (7, 1), (16, 8)])
def test_forced_splits_against_the_oracle_composition(gpu, H, Hkv, int4, splits):
    c = _ragged(H, Hkv, int4)
    box = _Canaried(c["T"], H, gpu)
    out = _attend(c, out=box.out, num_splits=splits)
    torch.cuda.synchronize()
    box.check()
    _spare_blocks_untouched(c["pools"], c["tables"], c["nblocks"])
    assert torch.equal(c["pools"].k, c["pages"][0]) and torch.equal(c["pools"].v, c["pages"][1]), "the attention wrote a page"
    err = _err(c, out, f"split append H={H} Hkv={Hkv} int4={int4} splits={splits}")
    assert err <= TOL, f"max abs err {err:.2e}"


# ---- 2. stale workspace ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("int4", KV)
def test_empty_splits_never_read_the_previous_calls_records(gpu, int4):
    """16 splits on the ragged batch fill the records of every split of the longest sequence; the next call on the same stream has 1
    to 2 pages per sequence, so 14 to 15 of its 16 splits are empty and their records are the first call's."""
    H, Hkv = 8, 2
    first = _ragged(H, Hkv, int4)
    second = _case(H, Hkv, int4, tuple(SHORT_PASTS), tuple(NS), 77 + int(int4))
    e1 = _err(first, _attend(first, num_splits=16), "16 splits, long pasts")
    e2 = _err(second, _attend(second, num_splits=16), "16 splits, 1 to 2 pages per sequence, same stream")
    assert e1 <= TOL and e2 <= TOL, (e1, e2)


# ---- 3. one split is today's kernel ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("int4", KV)
def test_one_split_is_the_unsplit_kernel_bit_for_bit(gpu, int4):
    from qserve_amd.plan import append_attention_split_plan
    c = _ragged(8, 2, int4)
    assert torch.equal(_attend(c, num_splits=1), c["unsplit"])
    # the wrapper with a hint on a shape where the planner answers 1 (a past under two pages)
    assert append_attention_split_plan(c["B"], c["msq"], 100, 8, 2, int4)["splits"] == 1
    assert torch.equal(_attend(c, max_past=100), c["unsplit"])


# ---- 4. the hint is only a hint ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("int4", KV)
@pytest.mark.parametrize("hint", [64, 1000, 10 ** 6])
def test_the_length_hint_does_not_decide_the_result(gpu, int4, hint):
    """True past 1000, B = 1, 8 / 2 heads, n = 8; the planner sees 64 (too small: one split), 1000, 10^6 (cut to the pointer table)."""
    from qserve_amd.plan import append_attention_split_plan
    c = _case(8, 2, int4, (1000,), (8,), 3 + int(int4))
    seen = min(hint, 64 * c["mb"])
    splits = append_attention_split_plan(1, 8, seen, 8, 2, int4)["splits"]
    assert (splits == 1) == (hint == 64) and splits <= 64
    out = _attend(c, max_past=hint)
    err = _err(c, out, f"hint {hint} -> {splits} splits")
    assert err <= TOL
    assert torch.equal(out, _attend(c, num_splits=splits)), "the hinted call differs from the forced call with the planner's count"


# ---- 5. planted keys decide the output ---------------------------------------------------------------------------------------------
def _planted_case(G, int4):
    """L = 513: past 512 = 8 pages, 8 splits of one page each, the new token with the last.  Sequence b < 8: the dominant key sits in
    split b; sequence 8: the new token dominates; sequence 9: a cached key dominates and the new token is negligible."""
    H, Hkv = AC.GQA[G]
    L = 513
    pl = {}
    for hk in range(Hkv):
        for b in range(8):
            pl[(b, hk, 64 * b + (7 * b + 5 + hk) % 64)] = 25.0
        pl[(8, hk, L - 1)] = 20.0
        pl[(9, hk, 300 + hk)] = 20.0
        pl[(9, hk, L - 1)] = -10.0
    return AC.decode_case(10, H, Hkv, L, int4, pl, seed=900 + G + 10 * int(int4))


@pytest.mark.parametrize("int4", KV)
@pytest.mark.parametrize("G", [1, 4, 8])
def test_planted_keys_in_each_split_decide_the_output(gpu, G, int4):
    from qserve_amd import append as A
    c = _planted_case(G, int4)
    H, Hkv, L, B = c["H"], c["Hkv"], c["L"], 10
    # on the host, before anything runs: removing a planted key moves the reference by >= SENS x the bar
    ex, _ = AC.decode_exact(c)
    for (b, hk, pos), level in c["planted"].items():
        if level <= 6.0:
            continue
        alt, _ = AC.decode_exact(c, drop=[(b, hk, pos)], only={b})
        moved = min(np.abs(alt[b, h] - ex[b, h]).max() for h in range(hk * G, hk * G + G))
        assert moved >= AC.SENS * TOL, (b, hk, pos, moved)
    pools = DevPools(c["nblocks"], Hkv, int4, gpu)
    pools.k.copy_(dev(c["pool"].k))
    pools.v.copy_(dev(c["pool"].v))
    new = np.concatenate([c["q"].reshape(B, -1), c["k"].reshape(B, -1), c["v"].reshape(B, -1)], axis=1)
    cu_q, past = np.arange(B + 1, dtype=np.int32), np.full(B, L - 1, np.int32)
    qkv = dev(new)
    out = A.append(qkv, dev(cu_q), dev(past), pools.pointers(c["tables"]), H, Hkv, _spt(Hkv, int4), AC.ROPE, int4, max_seqlen_q=1,
                   num_splits=8)
    torch.cuda.synchronize()
    ref = expected(rotate_rows(new, cu_q, past, H, Hkv, AC.ROPE), cu_q, past, c["tables"], c["pool"], H, Hkv)
    got = _np(out).astype(np.float32)
    assert np.isfinite(got).all()
    err = np.abs(got - ref).max(axis=(1, 2))
    print(f"planted G={G} int4={int4}: max abs err per sequence {np.array2string(err, precision=2)}")
    assert err.max() <= TOL, f"max abs err {err.max():.2e} (sequence {int(err.argmax())})"


# ---- 6. determinism and capture ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("int4", KV)
def test_forced_split_call_is_deterministic_and_capturable(gpu, int4):
    from qserve_amd import append as A
    c = _ragged(8, 2, int4)
    a = _attend(c, num_splits=7)
    b = _attend(c, num_splits=7)
    torch.cuda.synchronize()
    assert torch.equal(a, b)                              # (and the workspace exists now)
    # writer + split attention in one graph on one stream; the writer rotates qkv in place, so the graph starts from the raw rows
    qkv = torch.empty_like(c["src"])
    out = torch.zeros((c["T"], c["H"], 128), dtype=torch.float16, device=gpu)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        qkv.copy_(c["src"])
        A.append_rope_update_kv_cache(qkv, c["cu_q"], c["past"], c["kvp"], c["H"], c["Hkv"], c["spt"], BASE, int4)
        A.append_attention(qkv, c["cu_q"], c["past"], c["kvp"], c["H"], c["Hkv"], c["spt"], int4, max_seqlen_q=c["msq"], out=out,
                           num_splits=7)
    for _ in range(2):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, a), "replay differs from the eager call"
    assert torch.equal(qkv, c["qkv"])
    assert torch.equal(c["pools"].k, c["pages"][0]) and torch.equal(c["pools"].v, c["pages"][1])


_CHILD = r"""
import sys
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import numpy as np, torch
from _append_cases import expected, host_pool, scattered_tables
from _helpers import DevPools, dev
from qserve_amd import append as A
from qserve_backend import fused_attention as fa
gpu = torch.device("cuda:0")
H, Hkv, int4, past_len, n, BASE = 8, 2, True, 1000, 8, 1e4
spt = Hkv * 64
r = np.random.default_rng(5)
W = (H + 2 * Hkv) * 128
tables, nblocks = scattered_tables(r, 1, 17)
pools = DevPools(nblocks, Hkv, int4, gpu)
kvp = pools.pointers(tables)
ctx = dev(r.standard_normal((past_len, W)).astype(np.float16))
cu = dev(np.array([0, past_len], np.int32))
fa.apply_bias_rope_update_kv_cache(ctx, dev(np.array([past_len], np.int32)), fa.compute_padding_offsets(cu, past_len, past_len), kvp, H,
                                   Hkv, past_len, 64, spt, 128, BASE, 8192, True, int4, True)
qkv = dev(r.standard_normal((n, W)).astype(np.float16))
cu_q, past = dev(np.array([0, n], np.int32)), dev(np.array([past_len], np.int32))
A.append_rope_update_kv_cache(qkv, cu_q, past, kvp, H, Hkv, spt, BASE, int4)
out = torch.zeros((n, H, 128), dtype=torch.float16, device=gpu)
torch.cuda.synchronize()
g = torch.cuda.CUDAGraph()
with torch.cuda.graph(g):        # the FIRST split call of this process: no workspace yet, none may be allocated here
    A.append_attention(qkv, cu_q, past, kvp, H, Hkv, spt, int4, max_seqlen_q=n, out=out, num_splits=8)
g.replay()
torch.cuda.synchronize()
hp = host_pool(pools.k.cpu().numpy(), pools.v.cpu().numpy(), Hkv, int4)
ref = expected(qkv.cpu().numpy(), np.array([0, n], np.int32), np.array([past_len], np.int32), tables, hp, H, Hkv)
err = float(np.abs(out.cpu().numpy().astype(np.float32) - ref).max())
same = torch.equal(out, A.append_attention(qkv, cu_q, past, kvp, H, Hkv, spt, int4, max_seqlen_q=n))
print(f"CHILD err={err:.3e} unsplit={int(same)}")
"""


def test_first_call_inside_a_capture_falls_back_to_the_unsplit_launch(gpu):
    """A fresh process (the workspace is allocated lazily, once per process and device): started with subprocess, nothing re-executed."""
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, os.path.join(ROOT, "tests")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("CHILD")][-1]
    print(line)
    err, same = float(line.split("err=")[1].split()[0]), line.endswith("unsplit=1")
    assert err <= TOL, line
    assert same, "a first call inside a capture must be the un-split launch, bit for bit"


# ---- 7. layouts ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("int4", KV)
def test_padded_qkv_and_out_strides(gpu, int4):
    """qkv stride W + 8 (NaN in the padding), out stride H * 128 + 8 (0xA5 in the padding), 3 splits, through the C ABI."""
    from qserve_amd._lib import lib
    c = _ragged(8, 2, int4)
    H, T, W = c["H"], c["T"], c["W"]
    packed = _attend(c, num_splits=3)
    qs, os_ = W + 8, H * 128 + 8
    praw = torch.full(((T + 1) * qs,), 0x7E00, dtype=torch.int16, device=gpu)                 # fp16 NaN
    pq = praw.view(torch.float16).as_strided((T, W), (qs, 1), 8)
    pq.copy_(c["qkv"])
    snap = praw.clone()
    oraw = torch.full(((T + 1) * os_,), 0xA5A5 - 0x10000, dtype=torch.int16, device=gpu)
    po = oraw.view(torch.float16).as_strided((T, H * 128), (os_, 1), 16)
    inside = torch.zeros(oraw.numel(), dtype=torch.bool, device=gpu)
    inside.as_strided((T, H * 128), (os_, 1), 16).fill_(True)
    rc = lib.qs_append_attention_split(pq.data_ptr(), po.data_ptr(), c["cu_q"].data_ptr(), c["past"].data_ptr(), c["kvp"].data_ptr(), T,
                                       c["B"], c["msq"], c["mb"], H, c["Hkv"], 128, qs, os_, 64, c["spt"], int(int4), 1, -1, 3, None)
    assert rc == 0, lib.qs_last_error()
    torch.cuda.synchronize()
    got = po.reshape(T, H, 128)
    assert torch.equal(got, packed), "the padded call differs from the call on contiguous buffers"
    assert bool((oraw[~inside] == 0xA5A5 - 0x10000).all()), "a byte outside the out view was written"
    assert torch.equal(praw, snap), "the call wrote into qkv"
    assert _err(c, got, f"padded layouts int4={int4}") <= TOL
