"""GPU tests of `stopping.stop_update` (csrc/stop_update.hip) against the numpy restatement of tests/_stop_cases.py: the named cases in a
handful of launches of at most 8 sequences, random launches over a six-token vocabulary, exact equality of every output, untouched
inputs, and eager against a captured replay."""
import numpy as np
import pytest
import torch

from _stop_cases import gpu_cases, named_cases, restate_loop

pytestmark = pytest.mark.gpu

INPUTS = ("history", "lengths", "prompt_lens", "node_tokens", "accept_idx", "stop_seqs", "stop_lens", "limit_lens")
IN_OUT = ("accept_lens", "next_token", "last_row", "finished")


def _device(case, gpu):
    dev = {k: None if case[k] is None else torch.from_numpy(case[k].copy()).to(gpu) for k in INPUTS + IN_OUT}
    dev["store"] = dev["history"]
    dev["history"] = dev["store"][:, :case["cap"]]                          # (a view: the row stride is the padded one)
    return dev


def _launch(dev, case):
    from qserve_amd import stopping
    return stopping.stop_update(dev["history"], dev["lengths"], dev["next_token"], dev["finished"], dev["stop_seqs"], dev["stop_lens"],
                                dev["limit_lens"], dev["prompt_lens"], dev["node_tokens"], dev["accept_idx"], dev["accept_lens"], dev["last_row"],
                                check_root=bool(case["check_root"]))


def _check(name, case, dev, k):
    want = restate_loop(case)
    got = dict(accept_lens=k, next_token=dev["next_token"], last_row=dev["last_row"], finished=dev["finished"])
    for key in IN_OUT:
        g = got[key].cpu().numpy()
        bad = np.nonzero(g != want[key])[0]
        assert bad.size == 0, f"{name}: {key} of row {bad[0]} ({case['names'][bad[0]]}): {g[bad[0]]}, expected {want[key][bad[0]]}"
    for key in INPUTS:
        src = case[key]
        if src is not None:
            assert np.array_equal((dev["store"] if key == "history" else dev[key]).cpu().numpy(), src), f"{name}: the input {key} was written"


def test_the_kernel_is_the_rule_on_every_case(gpu):
    for name, case in gpu_cases().items():
        dev = _device(case, gpu)
        k = _launch(dev, case)
        assert k is dev["accept_lens"] or case["accept_lens"] is None
        _check(name, case, dev, k)


def test_eager_equals_captured_replay(gpu):
    """Two launches - a verification with every kind of outcome and a plain step - captured in one graph over copies of their inputs:
    the replay leaves what the eager launches left, and a second replay on restored inputs does so again."""
    cases = [named_cases()[n] for n in ("tree12", "tree64", "step")]
    eager = [_device(c, gpu) for c in cases]
    eager_k = [_launch(d, c).clone() for d, c in zip(eager, cases)]
    held = [_device(c, gpu) for c in cases]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                              # (a warm-up outside the capture, on copies of their own)
        for c in cases:
            _launch(_device(c, gpu), c)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ks = [_launch(d, c) for d, c in zip(held, cases)]
    for rnd in range(2):
        for d, c in zip(held, cases):                                       # restore the in / out tensors, in place
            for key in IN_OUT:
                if d[key] is not None:
                    d[key].copy_(torch.from_numpy(c[key]))
        g.replay()
        torch.cuda.synchronize()
        for i, (d, e, c) in enumerate(zip(held, eager, cases)):
            _check(f"replay {rnd}, launch {i}", c, d, ks[i])
            assert torch.equal(ks[i], eager_k[i])
            for key in ("next_token", "last_row", "finished"):
                assert torch.equal(d[key], e[key]), f"replay {rnd}, launch {i}: {key} differs from the eager launch"
