"""Sampled decoding in the engine: verify_tree(sampled=True) on the host path and with the device walk, capture_verify(sampled=True),
and the sampling head of step() - recomputed from the logits with the float64 oracle of tests/_sample_cases.py and a host walk, under
the acceptance rule of tests/test_sample_rows_gpu.py.

Setting: the tiny engine of tests/_accept_engine.py (B = 3, P = 70, seed 5), on KV4 and on KV8, and a 7-node tree whose nodes have 2, 1
and 0 children; node i of sequence b is keyed by (b, lengths[b] + depth(i)), the position of the token that follows it.

A verification only writes cache slots at and behind lengths - 1, which the next one overwrites before it reads them, so a test probes
the logits of a draft and then puts `tokens`, `lengths` and the host-side length bound back instead of building a new engine."""
import numpy as np
import pytest
import torch

import _accept_engine as E
from _sample_cases import Row, depths, philox_uniform, position_keys, walk

pytestmark = pytest.mark.gpu

PAR = [-1, 0, 0, 1, 3, 3, 4]             # children: node 0 has 2, node 1 has 1, node 3 has 2, node 4 has 1; nodes 2, 5, 6 have none
CHAIN = [1, 3, 4, 6]
DEP = depths(PAR)
T, K, TOP_P, SEED = 0.8, 50, 0.95, 17
N = len(PAR)


def _engine(gpu, int4):
    from qserve_amd.decode import TINY, DecodeEngine
    e = DecodeEngine(TINY, batch=E.B, prompt_len=E.P, max_new=40, device="cuda:0", seed=5, int4_kv=int4)
    e.prefill(E.P, E.prompt(gpu))
    e.set_sampling(T, K, TOP_P, seed=SEED)
    return e


def _save(e):
    return e.tokens.clone(), e.lengths.clone(), e._len_bound


def _restore(e, state):
    e.tokens.copy_(state[0])
    e.lengths.copy_(state[1])
    e._len_bound = state[2]


def _uniform(b, position):
    return float(philox_uniform(position_keys([b], [position]), SEED)[0])


def _recompute(e, draft, res, before):
    """The engine's result against the oracle: every node's sampled token is admissible for its logits row and its key's uniform; the
    host walk over the sampled tokens gives accept_idx / accept_lens; `tokens` is the token sampled at the last accepted node and
    `lengths` grew by the path's length.  -> the paths."""
    torch.cuda.synchronize()
    idx, lens, sampled = (t.cpu().numpy() for t in res)
    logits = e.last_verify_logits.cpu().numpy()
    tok0, len0 = before[0].cpu().numpy(), before[1].cpu().numpy()
    toks = draft.cpu().numpy().copy()
    toks[:, 0] = tok0
    paths = []
    for b in range(E.B):
        for i in range(N):
            u = _uniform(b, int(len0[b]) + DEP[i])
            assert Row(logits[b, i], T, K, TOP_P).accepts(sampled[b, i], u), f"sequence {b}, node {i}: token {sampled[b, i]}, u={u}"
        path, bonus = walk(PAR, toks[b].tolist(), sampled[b].tolist())
        assert lens[b] == len(path) and idx[b].tolist() == path + [0] * (N - len(path)), f"sequence {b}: {idx[b]}, {lens[b]} != {path}"
        assert int(e.tokens[b]) == bonus and int(e.lengths[b]) == len0[b] + len(path)
        paths.append(path)
    return paths


def _oracle_chain_draft(e, gpu, rng):
    """A draft whose nodes 1, 3, 4, 6 carry the oracle's own chain: node by node, the token the oracle draws from the logits of the
    node's parent.  A sibling of a chain node never carries the same token.  The engine is left as it was."""
    from qserve_amd.decode import TINY
    V = TINY["vocab"]
    state = _save(e)
    len0 = state[1].cpu().numpy()
    draft = torch.from_numpy(rng.integers(0, V, size=(E.B, N))).to(gpu)
    for node in CHAIN:
        e.verify_tree(draft, PAR, sampled=True)
        torch.cuda.synchronize()
        logits = e.last_verify_logits.cpu().numpy()
        _restore(e, state)
        for b in range(E.B):
            tok = Row(logits[b, PAR[node]], T, K, TOP_P).token(_uniform(b, int(len0[b]) + DEP[PAR[node]]))
            draft[b, node] = tok
            for sib in [c for c in range(N) if PAR[c] == PAR[node] and c != node]:
                draft[b, sib] = (tok + 1 + sib) % V
    return draft


@pytest.mark.parametrize("int4", [True, False], ids=["kv4", "kv8"])
def test_sampled_verify_host_and_device_walk(gpu, int4):
    """Random draft, the oracle's own chain (accepted to full depth) and a draft whose first children can never match (cut to the
    root): host path and device walk agree with each other and with the oracle's recomputation; then a second verification on the
    now ragged lengths."""
    e = _engine(gpu, int4)
    rng = np.random.default_rng(3)
    state = _save(e)
    forced = _oracle_chain_draft(e, gpu, rng)
    # the root's children carry the two least likely tokens of the root's row: outside the top-k, they can never be drawn
    e.verify_tree(forced, PAR, sampled=True)
    torch.cuda.synchronize()
    low = torch.argsort(e.last_verify_logits[:, 0, :].float(), dim=1)[:, :2]
    _restore(e, state)
    never = forced.clone()
    never[:, 1], never[:, 2] = low[:, 0], low[:, 1]
    for name, draft in (("random", E.random_draft(rng, gpu)[:, :N].contiguous()), ("never", never), ("forced", forced)):
        host = e.verify_tree(draft, PAR, sampled=True)
        paths = _recompute(e, draft, host, state)
        host_state = _save(e)
        _restore(e, state)
        dev = e.verify_tree(draft, PAR, device_walk=True, sampled=True)
        _recompute(e, draft, dev, state)
        E.assert_same_result(host, dev, name)
        assert torch.equal(e.tokens, host_state[0]) and torch.equal(e.lengths, host_state[1]), f"{name}: host path and device walk differ"
        if name == "never":
            assert all(len(p) == 1 for p in paths), paths
        if name == "forced":
            assert all(p == [0] + CHAIN for p in paths), f"the oracle's own chain was not accepted to full depth: {paths}"
        else:
            _restore(e, state)
    # go on from the (ragged only in the keys: every sequence advanced by 5) state, then from a ragged one
    e.sync_length_bound()
    state2 = _save(e)
    draft2 = E.random_draft(rng, gpu)[:, :N].contiguous()
    _recompute(e, draft2, e.verify_tree(draft2, PAR, sampled=True), state2)
    e.lengths.add_(torch.tensor([0, 2, 1], dtype=torch.int32, device=gpu))         # (the slots hold stale but well-formed K / V)
    e.sync_length_bound()
    state3 = _save(e)
    _recompute(e, draft2, e.verify_tree(draft2, PAR, device_walk=True, sampled=True), state3)
    with pytest.raises(AssertionError):
        e.set_sampling(None)
        e.verify_tree(draft2, PAR, sampled=True)


@pytest.mark.parametrize("int4", [True, False], ids=["kv4", "kv8"])
def test_sampled_step_eager_and_captured(gpu, int4):
    """set_sampling, then a captured step() run three times: every token is admissible for the logits of its step under the uniform of
    (sequence, position) - the captured step advances its own randomness -, and an eager twin draws the same tokens.  Back on greedy,
    the head is the arg-max again."""
    cap, twin = _engine(gpu, int4), _engine(gpu, int4)
    assert torch.equal(cap.tokens, twin.tokens)
    cap.capture()                                                   # (its warm-up is a real step)
    twin.step()
    seen = []
    for it in range(3):
        len0 = cap.lengths.cpu().numpy().copy()
        cap.run()
        twin.step()
        torch.cuda.synchronize()
        logits = torch.matmul(cap.final, cap.lm_head.t()).cpu().numpy()
        for b in range(E.B):
            u = _uniform(b, int(len0[b]))
            assert Row(logits[b], T, K, TOP_P).accepts(int(cap.tokens[b]), u), f"replay {it}, sequence {b}"
        assert torch.equal(cap.tokens, twin.tokens) and torch.equal(cap.lengths, twin.lengths), f"replay {it}: captured != eager"
        assert cap.lengths.cpu().numpy().tolist() == (len0 + 1).tolist()
        seen.append([_uniform(b, int(len0[b])) for b in range(E.B)])
    assert seen[0] != seen[1] != seen[2]
    # sampling set before the prefill: the prompt's head draws the first token, at position P
    from qserve_amd.decode import TINY, DecodeEngine
    first = DecodeEngine(TINY, batch=E.B, prompt_len=E.P, max_new=40, device="cuda:0", seed=5, int4_kv=int4)
    first.set_sampling(T, K, TOP_P, seed=SEED)
    first.prefill(E.P, E.prompt(gpu))
    torch.cuda.synchronize()
    logits = torch.matmul(first.final, first.lm_head.t()).cpu().numpy()
    assert first.lengths.tolist() == [E.P + 1] * E.B
    for b in range(E.B):
        assert Row(logits[b], T, K, TOP_P).accepts(int(first.tokens[b]), _uniform(b, E.P)), f"prefill, sequence {b}"
    twin.set_sampling(None)
    twin.step()
    torch.cuda.synchronize()
    assert torch.equal(twin.tokens, torch.matmul(twin.final, twin.lm_head.t()).float().argmax(dim=1))


@pytest.mark.parametrize("int4", [True, False], ids=["kv4", "kv8"])
def test_capture_verify_sampled_replays_against_eager(gpu, int4):
    """capture_verify(sampled=True) and two run_verify calls against a twin that makes the same calls eagerly from the same state;
    both against the oracle."""
    cap, twin = _engine(gpu, int4), _engine(gpu, int4)
    rng = np.random.default_rng(9)
    zero = torch.zeros((E.B, N), dtype=torch.int64, device=gpu)
    cap.capture_verify(PAR, sampled=True)                           # (its warm-up is a real verification of an all-zero draft)
    twin.verify_tree(zero, PAR, device_walk=True, sampled=True)
    E.assert_same_state(cap, twin, "after capture_verify")
    for i, draft in enumerate((_oracle_chain_draft(twin, gpu, rng), E.random_draft(rng, gpu)[:, :N].contiguous())):
        before = _save(twin)
        got = cap.run_verify(draft)
        want = twin.verify_tree(draft, PAR, device_walk=True, sampled=True)
        torch.cuda.synchronize()
        E.assert_same_result(got, want, f"replay {i}")
        E.assert_same_state(cap, twin, f"replay {i}")
        paths = _recompute(twin, draft, want, before)
        if i == 0:
            assert all(p == [0] + CHAIN for p in paths), paths
