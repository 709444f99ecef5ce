"""append.qk_norm_rows (csrc/qk_norm_rows.hip) against its rule in float64 with both fp16 roundings applied exactly: per head slice x,
t = fp16(x / sqrt(mean(x^2) + eps)), y = fp16(w * t).  Tolerance, derived: |got - ref| <= 2^-10 |ref| + 2^-24 - one fp16 ulp for a
rounding of t that flips on the kernel's float32 r, plus the subnormal step.  A flipped ulp of t is w * ulp(t) in y: ONE ulp of y only
where w * t is exact, up to two under a weight with a significand other than 1 (the rule's own float32 does that, in numpy too, about once in
2e5 elements).  So where a flip can happen the weights are signed powers of two - of period 3 over the dimensions, which no 8-half
lane chunk shares, k's being q's shifted and negated: the wrong vector or offset moves every element - and full significands are checked
where t is exact: a head of +-60 000 has t = +-1 and y = +-w bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
EPS, I = 1e-6, np.arange(128)
WQ = (2.0 ** (I % 3 - 1) * np.where(I % 2, -1.0, 1.0)).astype(np.float16)            # 0.5, -1, 2, -0.5, 1, -2, ...
WK = (-(2.0 ** ((I + 1) % 3 - 1)) * np.where(I % 2, -1.0, 1.0)).astype(np.float16)    # -1, 2, -0.5, 1, -2, 0.5, ...
W_FULL = np.random.default_rng(5).uniform(0.5, 1.5, (2, 128)).astype(np.float16)


def reference(rows, wq, wk, H, Hkv):
    """rows fp16 [T, stride] -> the same with the first H + Hkv heads of every row normalised."""
    out, T = rows.copy(), rows.shape[0]
    x = rows[:, :(H + Hkv) * 128].reshape(T, H + Hkv, 128).astype(np.float64)
    t = (x / np.sqrt((x * x).mean(-1, keepdims=True) + float(np.float32(EPS)))).astype(np.float16).astype(np.float64)
    w = np.concatenate([np.broadcast_to(wq, (H, 128)), np.broadcast_to(wk, (Hkv, 128))]).astype(np.float64)
    out[:, :(H + Hkv) * 128] = (w * t).astype(np.float16).reshape(T, -1)
    return out


def run(buf, wq, wk, H, Hkv, gpu="cuda:0"):
    """The call on the view of the first (H + 2 Hkv) * 128 columns of `buf` (numpy: copied to the device first) -> the whole buffer."""
    from qserve_amd import append
    buf = torch.from_numpy(buf).to(gpu) if isinstance(buf, np.ndarray) else buf
    view = buf[:, :(H + 2 * Hkv) * 128]
    assert append.qk_norm_rows(view, torch.from_numpy(wq).to(gpu), torch.from_numpy(wk).to(gpu), H, Hkv, EPS) is view
    return buf.cpu().numpy()


def assert_close(got, ref, what):
    g, r = got.astype(np.float64), ref.astype(np.float64)
    bad = ~(np.abs(g - r) <= 2.0 ** -10 * np.abs(r) + 2.0 ** -24)                       # (a NaN or an inf is bad)
    assert not bad.any(), f"{what}: {int(bad.sum())} elements off, the first at {np.argwhere(bad)[0]}: {g[bad][0]} for {r[bad][0]}"


@pytest.mark.parametrize("pad", [0, 64])
@pytest.mark.parametrize("H, Hkv", [(8, 2), (4, 4), (5, 1)])         # (5, 1): the q / k boundary falls inside a wave's four slots
@pytest.mark.parametrize("T", [1, 3, 17])                            # 17 tokens: the last workgroup's 16 slots are partly empty
def test_rows_match_the_rule(gpu, T, H, Hkv, pad):
    rng, k0 = np.random.default_rng(1000 * T + 10 * H + Hkv + pad), (H + Hkv) * 128
    rows = (rng.standard_normal((T, k0 + Hkv * 128 + pad)) * rng.uniform(0.01, 30.0, (T, 1))).astype(np.float16)
    got = run(rows, WQ, WK, H, Hkv)
    assert_close(got[:, :k0], reference(rows, WQ, WK, H, Hkv)[:, :k0], f"T={T} H={H} Hkv={Hkv} pad={pad}")
    assert np.array_equal(got[:, k0:].view(np.uint16), rows[:, k0:].view(np.uint16)), "the v heads or the padding were written"
    assert np.array_equal(run(rows, WQ, WK, H, Hkv).view(np.uint16), got.view(np.uint16)), "a second call gives other bits"


@pytest.mark.parametrize("kind", ["zero", "big", "subnormal", "single"])
def test_extreme_heads(gpu, kind):
    H, Hkv, T, rng = 2, 1, 2, np.random.default_rng(7)
    rows = rng.standard_normal((T, (H + 2 * Hkv) * 128)).astype(np.float16)
    heads = rows[:, :(H + Hkv) * 128].reshape(T, H + Hkv, 128)        # (a view: what is planted below lands in `rows`)
    heads[:] = {"zero": 0, "single": 0, "big": np.where(rng.random(heads.shape) < 0.5, -60000.0, 60000.0),   # squares beyond fp16
                "subnormal": rng.integers(-1023, 1024, heads.shape) * 2.0 ** -24}[kind]
    if kind == "single":                                             # one non-zero element among zeros, somewhere in every head
        for t, h in np.ndindex(T, H + Hkv):
            heads[t, h, rng.integers(128)] = rng.uniform(-8, 8)
    wq, wk = W_FULL if kind == "big" else (WQ, WK)
    got = run(rows, wq, wk, H, Hkv)
    assert_close(got, reference(rows, wq, wk, H, Hkv), kind)
    g = got[:, :(H + Hkv) * 128].reshape(T, H + Hkv, 128)
    assert kind != "zero" or (g == 0).all(), "an all-zero head must stay all zero"
    assert kind != "big" or np.array_equal(g, np.sign(heads) * np.repeat(np.stack([wq, wk]), [H, Hkv], 0)), "t = +-1: y is +-w itself"


def test_graph_replay_is_bit_equal_to_eager(gpu):
    from qserve_amd import append
    T, H, Hkv, rng = 17, 5, 1, np.random.default_rng(11)
    inputs = [(rng.standard_normal((T, (H + 2 * Hkv) * 128)) * s).astype(np.float16) for s in (1.0, 20.0, 0.05)]
    eager = [run(x, WQ, WK, H, Hkv) for x in inputs]
    buf, side = torch.from_numpy(inputs[0]).to(gpu), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                     # (a warm-up outside the capture)
        run(buf, WQ, WK, H, Hkv)
    torch.cuda.current_stream().wait_stream(side)
    wq, wk, g = torch.from_numpy(WQ).to(gpu), torch.from_numpy(WK).to(gpu), torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        append.qk_norm_rows(buf, wq, wk, H, Hkv, EPS)
    for x, want in zip(inputs, eager):                               # the input buffer is refilled in front of every replay
        buf.copy_(torch.from_numpy(x))
        g.replay()
        assert np.array_equal(buf.cpu().numpy().view(np.uint16), want.view(np.uint16))
