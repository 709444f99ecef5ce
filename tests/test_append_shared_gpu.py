"""GPU parity of shared-prefix append attention (qs_append_attention_shared; qserve_amd.append.append_attention_shared / append_shared,
DecodeEngine.prefill_shared): ragged groups with forced prefix / suffix split counts and the planner's against the float64
composition of the existing oracles on the ALIASED tables (tests/_append_cases.py, tests/_shared_cases.py) at the bar of
tests/test_append_gpu.py, nothing shared = the split entry bit for bit, decoy pages behind the members' own prefix entries, planted
keys that single out one record's weight in the merge, stale workspace contents, and the engine."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _attn_cases as AC
import _shared_cases as SC
from _append_cases import compose, expected, host_pool, rotate_rows
from _helpers import DevPools, dev
from oracle import kvattn

pytestmark = pytest.mark.gpu
TOL = 2e-3      # tests/test_append_gpu.py TOL: an fp16 MFMA attention against a float64 oracle on standard normal inputs
BASE = 1e4
KV = [pytest.param(True, id="kv4"), pytest.param(False, id="kv8")]
HEADS = [(8, 2), (4, 4), (7, 1), (16, 8)]


def _spt(Hkv, int4):
    return Hkv * (64 if int4 else 128)


def _np(t):
    return t.detach().cpu().numpy()


class _Canaried:
    """out [T, H, 128] fp16 between two 4 KiB areas of 0xA5 (the rows beyond T)."""

    def __init__(self, T, H, device):
        self.raw = torch.full((8192 + T * H * 256,), 0xA5, dtype=torch.uint8, device=device)
        self.out = self.raw[4096:4096 + T * H * 256].view(torch.float16).view(T, H, 128)

    def check(self):
        assert bool((self.raw[:4096] == 0xA5).all()) and bool((self.raw[-4096:] == 0xA5).all()), "write outside `out`"


@functools.lru_cache(maxsize=None)
def _case(H, Hkv, int4, sizes, prefixes, extras, ns, seed):
    """Every sequence's past written through its OWN table (existing prefill writer), the members' prefix entries aliased to the first
    member's, the append writer run on the new rows through the aliased tables (it writes at slots >= past >= prefix: own pages), and
    the oracle composition on the aliased and on the own (decoy) tables - once per configuration; the attention never writes a page."""
    from qserve_amd import append as A
    from qserve_backend import fused_attention as fa
    gpu = torch.device("cuda:0")
    r = np.random.default_rng(seed)
    lay = SC.layout(sizes, prefixes, extras, ns)
    pasts, cu_q = lay["pasts"], lay["cu_q"]
    B, W, T = len(ns), (H + 2 * Hkv) * 128, int(sum(ns))
    own, aliased, nblocks, mb = SC.tables_for(r, lay, ns)
    assert mb <= 8 and int(pasts.max()) <= 450
    pools = DevPools(nblocks, Hkv, int4, gpu)
    live = [b for b in range(B) if pasts[b] > 0]
    lens = [int(pasts[b]) for b in live]
    ctx = dev(r.standard_normal((sum(lens), W)).astype(np.float16))
    cu_ctx = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    fa.apply_bias_rope_update_kv_cache(ctx, dev(np.asarray(lens, np.int32)), fa.compute_padding_offsets(dev(cu_ctx), max(lens), sum(lens)),
                                       pools.pointers(own[live]), H, Hkv, max(lens), 64, _spt(Hkv, int4), 128, BASE, 8192, True, int4, True)
    kvp = pools.pointers(aliased)
    qkv = dev(r.standard_normal((T, W)).astype(np.float16))
    A.append_rope_update_kv_cache(qkv, dev(cu_q), dev(pasts), kvp, H, Hkv, _spt(Hkv, int4), BASE, int4)
    torch.cuda.synchronize()
    hp = host_pool(_np(pools.k), _np(pools.v), Hkv, int4)
    ref = expected(_np(qkv), cu_q, pasts, aliased, hp, H, Hkv)
    ref_own = expected(_np(qkv), cu_q, pasts, own, hp, H, Hkv)
    groups = A.shared_prefix_groups(sizes, prefixes, gpu, batch=B)
    return dict(H=H, Hkv=Hkv, int4=int4, spt=_spt(Hkv, int4), B=B, T=T, mb=mb, msq=int(max(ns)), mgt=int(lay["group_tokens"].max()), qkv=qkv,
                cu_q=dev(cu_q), past=dev(pasts), kvp=kvp, kvp_own=pools.pointers(own), pools=pools, pages=(pools.k.clone(), pools.v.clone()),
                groups=groups, sizes=sizes, ref=ref, ref_own=ref_own, max_prefix=int(max(prefixes)), max_suffix=int(max(extras)))


def _ragged(H, Hkv, int4):
    return _case(H, Hkv, int4, SC.SIZES, SC.PREFIXES, SC.EXTRAS, SC.NS, 13 * H + Hkv + int(int4))


def _attend(c, out=None, kvp=None, groups=None, **kw):
    from qserve_amd import append as A
    return A.append_attention_shared(c["qkv"], c["cu_q"], c["past"], c["kvp"] if kvp is None else kvp, c["H"], c["Hkv"], c["spt"], c["int4"],
                                     c["groups"] if groups is None else groups, max_seqlen_q=c["msq"], max_group_tokens=c["mgt"], out=out, **kw)


def _err(ref, out, what):
    got = _np(out).astype(np.float32)
    assert np.isfinite(got).all(), f"{what}: non-finite output"
    err = float(np.abs(got - ref).max())
    print(f"{what}: max abs err {err:.3e}")
    return err


# ---- 1. ragged groups against the oracle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("PS", [(1, 1), (2, 1), (3, 2), (5, 3), None], ids=["P1S1", "P2S1", "P3S2", "P5S3", "planner"])
@pytest.mark.parametrize("int4", KV)
@pytest.mark.parametrize("H,Hkv", HEADS)
def test_ragged_groups_against_the_oracle_composition(gpu, H, Hkv, int4, PS):
    """Groups of 5 / 1 / 3 with prefixes 192 / 0 / 64, pasts prefix + {0, 1, 63, 64, 130}, n in {0, 1, 7, 13, 20}: the first group's 41
    tokens cross a query tile at G = 4 (32 tokens) and G = 7 (18) and a wave (32 rows) at every G; P = 5 over 3 pages holds empty
    prefix splits."""
    c = _ragged(H, Hkv, int4)
    box = _Canaried(c["T"], H, gpu)
    kw = dict(num_prefix_splits=PS[0], num_suffix_splits=PS[1]) if PS else dict(max_prefix=c["max_prefix"], max_suffix_past=c["max_suffix"])
    out = _attend(c, out=box.out, **kw)
    torch.cuda.synchronize()
    box.check()
    assert torch.equal(c["pools"].k, c["pages"][0]) and torch.equal(c["pools"].v, c["pages"][1]), "the attention wrote a page"
    err = _err(c["ref"], out, f"shared append H={H} Hkv={Hkv} int4={int4} (P, S)={PS}")
    assert err <= TOL, f"max abs err {err:.2e}"


# ---- 2. nothing shared: the split entry ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("int4", KV)
@pytest.mark.parametrize("S", [2, 3])
def test_it_is_the_split_entry_when_nothing_is_shared(gpu, int4, S):
    from qserve_amd import append as A
    c = _ragged(8, 2, int4)
    split = A.append_attention(c["qkv"], c["cu_q"], c["past"], c["kvp"], 8, 2, c["spt"], int4, max_seqlen_q=c["msq"], num_splits=S)
    assert torch.equal(_attend(c, num_prefix_splits=-1, num_suffix_splits=S), split), "`do not share` differs from the split entry"
    # all prefixes 0 through the two-role kernel and its merge: every prefix workgroup is empty, the suffix role walks the whole past
    zero = A.shared_prefix_groups(c["sizes"], [0] * len(c["sizes"]), c["qkv"].device)
    for P in (1, 3):
        assert torch.equal(_attend(c, groups=zero, num_prefix_splits=P, num_suffix_splits=S), split), f"prefixes 0, P = {P}"


# ---- 3. sharing is real -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("int4", KV)
@pytest.mark.parametrize("P", [1, 3])
def test_prefix_pages_are_read_through_the_first_members_table(gpu, int4, P):
    """White box, the documented rule: with P >= 1 in effect the members' own prefix entries are never followed.  Here they name pages
    of their own with DIFFERENT valid quantised data (each member's context written through its own table: finite scales, a decoy,
    not a fault); the result is still the oracle's on tables aliased to the first member, and not the oracle's on the decoy tables."""
    c = _ragged(8, 2, int4)
    _attend(c, num_prefix_splits=P, num_suffix_splits=1)
    torch.cuda.synchronize()                              # (eager: the workspace exists now)
    out = _attend(c, kvp=c["kvp_own"], num_prefix_splits=P, num_suffix_splits=1)
    got = _np(out).astype(np.float32)
    err = _err(c["ref"], out, f"decoy tables, P={P} int4={int4}")
    assert err <= TOL
    far = np.abs(got - c["ref_own"]).max(axis=(1, 2))
    print(f"distance from the oracle on the decoy tables: {far.max():.3e}; rows beyond the bar: {(far > TOL).sum()} of {len(far)}")
    assert (far > TOL).any(), "the result follows the members' own prefix entries"


# ---- 3b. no workspace yet: the un-split launch ------------------------------------------------------------------------------------------
_CHILD = r"""
import sys
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import numpy as np, torch
import _shared_cases as SC
from _append_cases import expected, host_pool
from _helpers import DevPools, dev
from qserve_amd import append as A
from qserve_backend import fused_attention as fa
gpu = torch.device("cuda:0")
H, Hkv, int4, BASE = 8, 2, True, 1e4
sizes, prefixes, extras, ns = (2,), (128,), (72, 72), (3, 3)      # one group of two, prefix 128 of past 200 (4 pages), n = 3
spt = Hkv * 64
r = np.random.default_rng(7)
W = (H + 2 * Hkv) * 128
lay = SC.layout(sizes, prefixes, extras, ns)
pasts, cu_np = lay["pasts"], lay["cu_q"]
own, aliased, nblocks, mb = SC.tables_for(r, lay, ns)
pools = DevPools(nblocks, Hkv, int4, gpu)
lens = [int(p) for p in pasts]
ctx = dev(r.standard_normal((sum(lens), W)).astype(np.float16))
cu_ctx = dev(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32))
fa.apply_bias_rope_update_kv_cache(ctx, dev(np.asarray(lens, np.int32)), fa.compute_padding_offsets(cu_ctx, max(lens), sum(lens)),
                                   pools.pointers(own), H, Hkv, max(lens), 64, spt, 128, BASE, 8192, True, int4, True)
kvp = pools.pointers(aliased)
qkv = dev(r.standard_normal((sum(ns), W)).astype(np.float16))
cu_q, past = dev(cu_np), dev(pasts)
A.append_rope_update_kv_cache(qkv, cu_q, past, kvp, H, Hkv, spt, BASE, int4)
groups = A.shared_prefix_groups(sizes, prefixes, gpu, batch=len(ns))
out = torch.zeros((sum(ns), H, 128), dtype=torch.float16, device=gpu)
torch.cuda.synchronize()
g = torch.cuda.CUDAGraph()
with torch.cuda.graph(g):        # the FIRST call of this process that wants the workspace: none yet, none may be allocated here
    A.append_attention_shared(qkv, cu_q, past, kvp, H, Hkv, spt, int4, groups, max_seqlen_q=3, max_group_tokens=6, out=out,
                              num_prefix_splits=2, num_suffix_splits=2)
g.replay()
torch.cuda.synchronize()
hp = host_pool(pools.k.cpu().numpy(), pools.v.cpu().numpy(), Hkv, int4)
ref = expected(qkv.cpu().numpy(), cu_np, pasts, aliased, hp, H, Hkv)
err = float(np.abs(out.cpu().numpy().astype(np.float32) - ref).max())
same = torch.equal(out, A.append_attention(qkv, cu_q, past, kvp, H, Hkv, spt, int4, max_seqlen_q=3))
print(f"CHILD err={err:.3e} unsplit={int(same)}")
"""


def test_first_call_inside_a_capture_falls_back_to_the_unsplit_launch(gpu):
    """tests/test_append_split_gpu.py's rule for this entry's own fall-back, in a fresh process (the workspace is allocated lazily, once
    per process and device): P = 2, S = 2 asked for, the linear un-split launch runs."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _CHILD, root, os.path.join(root, "tests")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("CHILD")][-1]
    print(line)
    err, same = float(line.split("err=")[1].split()[0]), line.endswith("unsplit=1")
    assert err <= TOL, line
    assert same, "a first call inside a capture must be the un-split launch, bit for bit"


# ---- 4. planted keys ----------------------------------------------------------------------------------------------------------------------
def _planted_case(G, int4):
    """Five groups of three sequences, prefix 192 (three pages: P = 3 gives one page per prefix split), one own page (past 256) and
    one new token.  The construction of tests/_attn_cases.py's decode_case: q = s * U + noise, background keys of small norm, a planted
    key a * U scores `level` nats, its value is +-0.75.  The members of a group share U, so a key planted in the (first member's)
    prefix decides every member's row.  Group g < 3: the key sits in prefix page g; group 3: in the own page of the first and of the
    last member; group 4: the new token of the first and of the last member."""
    H, Hkv = AC.GQA[G]
    r = np.random.default_rng(700 + G + 10 * int(int4))
    s, D, level = 2.0, 128, 25.0
    sizes, prefixes, extras, ns = (3,) * 5, (192,) * 5, (64,) * 15, (1,) * 15
    lay = SC.layout(sizes, prefixes, extras, ns)
    own, aliased, nblocks, mb = SC.tables_for(r, lay, ns)
    B, W, past = 15, (H + 2 * Hkv) * 128, 256
    a = level / (s * np.sqrt(D))
    sign = lambda: r.choice([-1.0, 1.0], D)               # noqa: E731
    ctx = np.zeros((B, past, W), np.float16)
    new = np.zeros((B, W), np.float16)
    planted = []                                          # (sequence the rows belong to, KV head, key position, table row that holds it)
    for g in range(5):
        U = np.stack([sign() for _ in range(Hkv)])
        for m in range(3):
            b = 3 * g + m
            K = r.normal(0, 0.15, (past + 1, Hkv, D))
            V = r.uniform(-0.25, 0.25, (past + 1, Hkv, D))
            for hk in range(Hkv):
                where = None
                if g < 3 and m == 0:
                    where = 64 * g + (7 * g + 5 + hk) % 64
                elif g == 3 and m != 1:
                    where = 192 + (11 + hk + m) % 64
                elif g == 4 and m != 1:
                    where = past
                if where is not None:
                    K[where, hk], V[where, hk] = a * U[hk], 0.75 * sign()
                    planted += [(bb, hk, where) for bb in ((3 * g, 3 * g + 2) if g < 3 else (b,))]
            qr = np.repeat(s * U, H // Hkv, axis=0) + r.normal(0, 0.05, (H, D))
            new[b, : H * D] = kvattn.rope_neox_inv(qr.astype(np.float16), past, AC.ROPE).reshape(-1)
            for t in range(past + 1):
                row = ctx[b, t] if t < past else new[b]
                row[H * D: (H + Hkv) * D] = kvattn.rope_neox_inv(K[t].astype(np.float16), t, AC.ROPE).reshape(-1)
                row[(H + Hkv) * D:] = V[t].astype(np.float16).reshape(-1)
    pool = kvattn.PagePool(nblocks, Hkv, D, int4, fill=0)
    lens = np.full(B, past, np.int32)
    cu_ctx = (np.arange(B + 1) * past).astype(np.int32)
    kvattn.prefill_update_kv_cache(ctx.reshape(B * past, W), lens, kvattn.compute_padding_offsets(cu_ctx, past, B * past), own, pool, H, Hkv,
                                   past, AC.ROPE)
    return dict(H=H, Hkv=Hkv, int4=int4, B=B, past=past, new=new, pool=pool, nblocks=nblocks, aliased=aliased, lay=lay, sizes=sizes,
                prefixes=prefixes, planted=planted)


@pytest.mark.parametrize("int4", KV)
@pytest.mark.parametrize("G", [1, 4, 8])
def test_planted_keys_in_each_record_decide_the_output(gpu, G, int4):
    from qserve_amd import append as A
    c = _planted_case(G, int4)
    H, Hkv, B, past = c["H"], c["Hkv"], c["B"], c["past"]
    cu_q, pl = np.arange(B + 1, dtype=np.int32), np.full(B, past, np.int32)
    rot = rotate_rows(c["new"], cu_q, pl, H, Hkv, AC.ROPE)
    ref = expected(rot, cu_q, pl, c["aliased"], c["pool"], H, Hkv)
    # on the host, before anything runs: removing a planted key moves the rows it decides by >= SENS x the bar
    q, K, V, cu_k = compose(rot, cu_q, pl, c["aliased"], c["pool"], H, Hkv)
    for b, hk, pos in c["planted"]:
        keys = int(cu_k[b]) + np.delete(np.arange(past + 1), pos)
        for h in range(hk * G, hk * G + G):
            sc = K[keys, hk].astype(np.float64) @ q[b, h].astype(np.float64) / np.sqrt(128)
            e = np.exp(sc - sc.max())
            moved = np.abs(e @ V[keys, hk].astype(np.float64) / e.sum() - ref[b, h]).max()
            assert moved >= AC.SENS * TOL, (b, hk, pos, moved)
    assert {b % 3 for b, _, _ in c["planted"]} == {0, 2} and len({b // 3 for b, _, _ in c["planted"]}) == 5   # first and last member, every group
    pools = DevPools(c["nblocks"], Hkv, int4, gpu)
    pools.k.copy_(dev(c["pool"].k))
    pools.v.copy_(dev(c["pool"].v))
    groups = A.shared_prefix_groups(c["sizes"], c["prefixes"], gpu, batch=B)
    out = A.append_shared(dev(c["new"]), dev(cu_q), dev(pl), pools.pointers(c["aliased"]), H, Hkv, _spt(Hkv, int4), AC.ROPE, int4, groups,
                          max_seqlen_q=1, max_group_tokens=3, num_prefix_splits=3, num_suffix_splits=1)
    torch.cuda.synchronize()
    got = _np(out).astype(np.float32)
    assert np.isfinite(got).all()
    err = np.abs(got - ref).max(axis=(1, 2))
    print(f"planted G={G} int4={int4}: max abs err per sequence {np.array2string(err, precision=2)}")
    assert err.max() <= TOL, f"max abs err {err.max():.2e} (sequence {int(err.argmax())})"


# ---- 5. stale workspace ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("int4", KV)
def test_stale_records_of_other_shapes_are_never_read(gpu, int4):
    """A larger shared call (the ragged batch, P = 5, S = 3) leaves its records; the smaller call with other group shapes that follows
    has empty prefix and suffix splits whose blocks hold that call's data.  Its result is the one it gives after a call of a third
    shape has filled the records with something else - and the oracle's."""
    H, Hkv = 8, 2
    big = _ragged(H, Hkv, int4)
    small = _case(H, Hkv, int4, (2, 2), (64, 128), (0, 70, 1, 64), (3, 0, 9, 2), 91 + int(int4))
    third = _case(H, Hkv, int4, (4,), (128,), (130, 0, 64, 5), (20, 20, 20, 20), 57 + int(int4))
    assert _err(big["ref"], _attend(big, num_prefix_splits=5, num_suffix_splits=3), "the larger call") <= TOL
    first = _attend(small, num_prefix_splits=5, num_suffix_splits=3)
    assert _err(third["ref"], _attend(third, num_prefix_splits=2, num_suffix_splits=3), "the third shape") <= TOL
    again = _attend(small, num_prefix_splits=5, num_suffix_splits=3)
    torch.cuda.synchronize()
    assert _err(small["ref"], first, "the smaller call behind the larger one") <= TOL
    assert torch.equal(first, again), "the result depends on what the previous call left in the workspace"


# ---- 6. the engine ------------------------------------------------------------------------------------------------------------------------
def test_engine_prefill_shared(gpu, monkeypatch):
    """prefill_shared(prefix 130, suffix 40, chunk 32) against prefill_chunked(170, 32) on the concatenated tokens, same seed: the same
    chunk boundaries (0, 32, .. 160), so layer 0's K / V - per-row-deterministic ops only - are byte-equal wherever both engines
    store them.  Attention tolerance of tests/test_append_gpu.py::test_engine_prefill_chunked (4e-3), here between every
    append_shared call and the un-split attention on the same rotated rows and (aliased) tables.  `hidden`: the two engines differ
    by fp32 summation order in the attention only, i.e. by fp16 roundings of its output (2^-11 relative) that the four int8
    re-quantisations per layer can turn into single quantisation steps (1 / 127 of a row's maximum) of a few values - bounded here by
    2.5 such steps of the largest state: 2e-2 * max |hidden|."""
    from qserve_amd import append as A
    from qserve_amd.decode import TINY, DecodeEngine
    P, S, CH, B = 130, 40, 32, 3
    g = torch.Generator(device=gpu).manual_seed(3)
    prefix = torch.randint(0, TINY["vocab"], (P,), device=gpu, generator=g)
    suffix = torch.randint(0, TINY["vocab"], (B, S), device=gpu, generator=g)
    toks = torch.cat([prefix.unsqueeze(0).expand(B, -1), suffix], dim=1).reshape(-1)
    ref = DecodeEngine(TINY, batch=B, prompt_len=P + S, max_new=8, device="cuda:0", seed=5)
    ref.prefill_chunked(P + S, CH, toks)
    eng = DecodeEngine(TINY, batch=B, prompt_len=P + S, max_new=8, device="cuda:0", seed=5)
    real, calls = A.append_shared, []

    def checked(qkv, cu_seqlens_q, past_lens, kv_pointers, num_heads, num_kv_heads, size_per_token, rope_theta, int4_kv, groups, **kw):
        assert groups[0].tolist() == [0, B] and groups[1].tolist() == [128] and groups[2].tolist() == [0] * B
        assert past_lens.tolist() == [128 + CH * (len(calls) // TINY["layers"])] * B
        out = real(qkv, cu_seqlens_q, past_lens, kv_pointers, num_heads, num_kv_heads, size_per_token, rope_theta, int4_kv, groups, **kw)
        un = A.append_attention(qkv, cu_seqlens_q, past_lens, kv_pointers, num_heads, num_kv_heads, size_per_token, int4_kv,
                                max_seqlen_q=kw["max_seqlen_q"])
        calls.append((out.float() - un.float()).abs().max().item())
        assert calls[-1] <= 4e-3, f"call {len(calls)}: shared vs un-split attention {calls[-1]:.2e}"
        return out

    monkeypatch.setattr(A, "append_shared", checked)
    eng.prefill_shared(prefix, suffix, chunk=CH)
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert len(calls) == TINY["layers"] * 2               # tokens 128 .. 159 and 160 .. 169
    print(f"engine: append_shared vs un-split attention, max over {len(calls)} calls {max(calls):.3e}")
    pb = eng.page_bytes
    for li in range(TINY["layers"]):
        tab = eng.tables[li]
        assert torch.equal(tab[:, :, :2], tab[0:1, :, :2].expand(B, -1, -1)), f"layer {li}: prefix entries are not sequence 0's"
    # layer 0, byte for byte: sequence 0's pages 0 and 1 (positions < 128), every sequence's pages from 2 on (positions >= 128)
    for which in (0, 1):
        e_idx = (eng.tables[0][:, which] - eng.pools[0][which].data_ptr()) // pb       # block indices [B, mb], on the device
        r_idx = (ref.tables[0][:, which] - ref.pools[0][which].data_ptr()) // pb
        assert torch.equal(eng.pools[0][which][e_idx[0, :2]], ref.pools[0][which][r_idx[0, :2]]), "positions < 128 of sequence 0"
        npages = (P + S + 63) // 64
        for b in range(B):
            assert torch.equal(eng.pools[0][which][e_idx[b, 2:npages]], ref.pools[0][which][r_idx[b, 2:npages]]), f"positions >= 128, sequence {b}"
    assert eng.lengths.tolist() == ref.lengths.tolist() == [P + S + 1] * B
    assert bool(torch.isfinite(eng.hidden).all())
    d = (eng.hidden.float() - ref.hidden.float()).abs().max().item()
    scale = ref.hidden.float().abs().max().item()
    print(f"engine: |hidden - prefill_chunked's| max {d:.3e} at max |hidden| {scale:.3e}")
    assert d <= 2e-2 * scale
    assert bool(((eng.tokens >= 0) & (eng.tokens < TINY["vocab"])).all())
    eng.step()
    torch.cuda.synchronize()
    eng.check()
    assert eng.lengths.tolist() == [P + S + 2] * B
