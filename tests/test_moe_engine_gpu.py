"""DecodeEngine on a mixture-of-experts config (TINY_MOE, B = 3; tests/_moe_engine.py): the fast path against the slow twin behind the
`moe.moe_mlp` seam on every path, bit for bit; that the routing decides something; what refuses; that a dense engine is what it was.  The
capture case runs tests/_moe_engine.py in a fresh process."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


@pytest.mark.parametrize("group_size", [-1, 128], ids=["per_chn", "g128"])
def test_fast_path_against_the_slow_twin(gpu, group_size):
    """prefill, prefill_chunked(16), two step()s, a device-walk verify_tree (its result and logits too) and a speculate() round: tokens,
    lengths, hidden and every K / V pool of the fast engine equal the slow twin's, bit for bit."""
    import _accept_engine as E
    import _moe_engine as M
    import _speculate_engine as S
    toks = E.prompt(gpu)
    calls = []
    with M.seam(lambda original, *a: (calls.append(a[0].size(0)), original(*a))[1]):
        a = M.moe_engine(toks, group_size=group_size)
    assert calls == [E.B * E.P] * len(a.layers), "the engine did not look moe.moe_mlp up per call"
    b = M.slow(lambda: M.moe_engine(toks, group_size=group_size))
    E.assert_same_state(a, b, "prefill")
    for i in range(2):
        a.step()
        M.slow(b.step)
        E.assert_same_state(a, b, f"step {i}")
    draft = E.random_draft(np.random.default_rng(7), gpu)
    ra = a.verify_tree(draft, E.PAR, device_walk=True)
    rb = M.slow(lambda: b.verify_tree(draft, E.PAR, device_walk=True))
    E.assert_same_result(ra, rb, "verify_tree")
    E.assert_same_state(a, b, "verify_tree")
    assert _same_bits(a.last_verify_logits, b.last_verify_logits), "verify_tree: the logits differ"
    if group_size != -1:
        return
    a2, b2 = M.moe_engine(toks, drafting=True), M.slow(lambda: M.moe_engine(toks, drafting=True))
    ra, rb = a2.speculate(E.PAR), M.slow(lambda: b2.speculate(E.PAR))
    E.assert_same_result(ra, rb, "speculate")
    E.assert_same_state(a2, b2, "speculate")
    S.assert_same_text(a2, b2, "speculate")
    assert _same_bits(a2.last_verify_logits, b2.last_verify_logits), "speculate: the logits differ"
    E.assert_same_state(M.moe_engine(toks, chunk=16), M.slow(lambda: M.moe_engine(toks, chunk=16)), "prefill_chunked")


def test_routing_decides_something(gpu):
    """Across the prompt at least three experts are used (layer 0's first call), and zeroing one expert's w2 scales changes exactly the
    rows routed to it."""
    import _accept_engine as E
    import _moe_engine as M
    toks = E.prompt(gpu)
    victim = 1

    def first_call(zero):
        seen = []

        def record(original, out, x, x_scale, x_sum, logits, k, gate_up, down, bufs):
            res = original(out, x, x_scale, x_sum, logits, k, gate_up, down, bufs)
            if not seen:
                seen.append((bufs["route"][0].clone(), out.clone()))
            return res

        e = M.moe_engine(toks, prefill=False)
        if zero:
            e.layers[0]["down"].s1_scales[victim].zero_()
            e.layers[0]["down"].s1_szeros[victim].zero_()
        with M.seam(record):
            e.prefill(E.P, toks)
        torch.cuda.synchronize()
        return seen[0]

    (ids, out), (ids0, out0) = first_call(False), first_call(True)
    assert torch.equal(ids, ids0) and tuple(ids.shape) == (E.B * E.P, 2)
    used = torch.unique(ids).tolist()
    assert len(used) >= 3 and victim in used, f"experts used across the prompt: {used}"
    routed = (ids == victim).any(dim=1)
    changed = (out.view(torch.int16) != out0.view(torch.int16)).any(dim=1)
    assert 0 < int(routed.sum()) < routed.numel()
    assert torch.equal(changed, routed), f"{int((changed & ~routed).sum())} rows changed that were not routed to expert {victim}, " \
                                         f"{int((routed & ~changed).sum())} routed rows did not change"


def test_what_refuses(gpu):
    import _accept_engine as E
    import _moe_engine as M
    from qserve_amd.decode import TINY_MOE, DecodeEngine
    with pytest.raises(AssertionError, match="mixture-of-experts config runs on one GPU"):
        DecodeEngine(TINY_MOE, batch=E.B, prompt_len=E.P, max_new=8, device="cuda:0", seed=5, tp_rank=0, tp_world=2)
    e = M.moe_engine(None, prefill=False)
    with pytest.raises(AssertionError, match="enable_lora: LoRA over expert weights is not built"):
        e.enable_lora(2, 16)
    with pytest.raises(AssertionError, match="set_lora: LoRA over expert weights is not built"):
        e.set_lora([0, 0, 0])
    assert e.planes == {} and e.moe == (4, 2)


def _digest(e):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in [e.tokens, e.lengths, e.hidden] + [p for kv in e.pools for p in kv]:
        h.update(t.contiguous().view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()


def test_a_dense_engine_is_what_it_was(gpu):
    """A dense TINY engine (no `experts` in its config): the digest of tokens, lengths, hidden and every K / V pool after prefill, two
    step()s and a device-walk verify_tree equals the one recorded on the commit before mixture of experts existed
    (tests/golden/moe_dense_state.json)."""
    import _accept_engine as E
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "moe_dense_state.json")))
    toks = E.prompt(gpu)
    e = E.engine(toks)
    assert e.moe is None and e.moe_bufs is None
    got = {"prefill": _digest(e)}
    e.step()
    e.step()
    got["two steps"] = _digest(e)
    e.verify_tree(E.random_draft(np.random.default_rng(7), gpu), E.PAR, device_walk=True)
    got["verify_tree"] = _digest(e)
    got["tokens"] = e.tokens.tolist()
    assert got == {k: want[k] for k in got}


def test_captured_step_and_round_replay_against_the_slow_twin(gpu):
    """tests/_moe_engine.py `capture` in a fresh process under a time limit of its own: capture() and three run()s against three eager
    steps of the slow twin, then one capture_speculate round likewise - no routing value reaches the host."""
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tests", "_moe_engine.py"), "capture"], cwd=ROOT,
                       capture_output=True, text=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and "MOE-CAPTURE-OK" in r.stdout, f"exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
