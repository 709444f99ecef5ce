"""The calls `DecodeEngine` makes into the C ABI, entry by entry, against a recorded golden (tests/golden/engine_traces.json).

Every symbol of `qserve_amd._lib.SIGNATURES` is wrapped on `lib` with a recorder, on top of the host-memory simulator of
tests/_fake_abi.py: entries the simulator has keep its arithmetic, the others become stubs that return 0 - three of them write the
smallest valid answer, because the engine goes on from what they return (the accept walk: the root alone; the drafter: the pad token;
the sampler: token 0).  A trace line is the entry's name (without `qs_`), every scalar argument, and for every pointer argument the
engine tensor whose storage holds the address, as `name+byte offset` - `layers[1].ln1`, `q_act`, `bufs.qa` (the `_prompt_buffers` of
the running call), `tables[0]`, `history` ... -, `tmp` for anything else and `0` for null.  No address and no tensor value reaches the
file.  The tree constants of `_tree_cache` are left unnamed on purpose: whether a verification builds or caches them is not part of the
call sequence.  Two seams above the C ABI add lines of their own: the `generate` scenario replaces the engine's `_capture(fn, advance)`
with a stand-in that writes `capture`, calls fn once and replays by calling it again, so that generate / run / run_speculate run on the
host; the LoRA scenario records the `lora_rows` calls where the engine makes them (the wrapper insists on a device workspace).

The golden is a table of the distinct lines plus, per scenario, the indices into it.  `python tests/test_engine_trace_cpu.py --record
[--decode FILE]` rewrites it; FILE is another revision of qserve_amd/decode.py to record from (it is loaded as a module of the
package), which is how a refactoring of the engine is held to the sequence of the revision before it."""
import argparse
import importlib
import importlib.util
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "engine_traces.json")
PAR = [-1, 0, 0, 1, 1, 2]                      # six nodes, two branchings
MAX_GOLDEN_BYTES = 72737                       # the largest golden the repository held before this one
# what a capture notes about its graph (result, kept tensors, private buffers) - tuples under these names in the revisions that kept
# it in engine attributes - is left unnamed like `_tree_cache`: where the engine keeps it is not part of the call sequence
CAPTURE_BOOKKEEPING = ("_graph_", "_verify_", "_speculate_")


# ---- the three stubs the engine goes on from ---------------------------------------------------------------------------------------
def _accept_root(tokens, argmax, parents, cu, T, batch, max_accept, accept_idx, accept_lens, last_row, next_token, stream):
    import _fake_abi as F
    F._arr(accept_idx, (batch, max_accept), np.int32)[:] = 0
    F._arr(accept_lens, (batch,), np.int32)[:] = 1
    F._arr(last_row, (batch,), np.int64)[:] = F._arr(cu, (batch + 1,), np.int32)[:batch]
    F._arr(next_token, (batch,), np.int64)[:] = 0
    return 0


def _draft_pad(history, stride, cap, lengths, parents, B, n, max_ngram, min_match, pad_token, out, stream):
    import _fake_abi as F
    F._arr(out, (B, n), np.int64)[:] = pad_token
    return 0


def _sample_zero(logits, out, rows, *rest):
    import _fake_abi as F
    F._arr(out, (rows,), np.int64)[:] = 0
    return 0


STEERING = {"qs_tree_accept_greedy": _accept_root, "qs_ngram_draft_tree": _draft_pad, "qs_sample_rows": _sample_zero}


# ---- the recorder ------------------------------------------------------------------------------------------------------------------
def _tensors(obj, name, out):
    if isinstance(obj, torch.Tensor):
        out.append((name, obj))
    elif isinstance(obj, dict):
        for k, v in obj.items():
            _tensors(v, f"{name}.{k}", out)
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            _tensors(v, f"{name}[{i}]", out)
    elif hasattr(obj, "qweight"):                                        # a W4A8Linear
        for k, v in vars(obj).items():
            _tensors(v, f"{name}.{k}", out)


class Recorder:
    def __init__(self):
        self.lines, self.eng, self.bufs = [], None, None

    def watch(self, eng):
        """Name pointers after `eng`'s tensors from here on, and after the `_prompt_buffers` of its running call."""
        self.eng, self.bufs = eng, None
        make = eng._prompt_buffers

        def prompt_buffers(T):
            self.bufs = make(T)                                          # (kept alive until the next call: its addresses are not reused)
            return self.bufs

        eng._prompt_buffers = prompt_buffers
        return eng

    def _ranges(self):
        found = []
        for attr, v in vars(self.eng).items():
            if attr != "_tree_cache" and not attr.startswith(CAPTURE_BOOKKEEPING):
                _tensors(v, attr, found)
        _tensors(self.bufs, "bufs", found)
        best = {}
        for name, t in found:
            st = t.untyped_storage()
            if st.nbytes() and (st.data_ptr() not in best or (len(name), name) < (len(best[st.data_ptr()][0]), best[st.data_ptr()][0])):
                best[st.data_ptr()] = (name, st.nbytes())
        return best

    def pointer(self, a, ranges):
        a = getattr(a, "value", a)
        if not a:
            return "0"
        if isinstance(a, int):
            for base, (name, size) in ranges.items():
                if base <= a < base + size:
                    return name if a == base else f"{name}+{a - base}"
        return "tmp"

    def wrap(self, symbol, fn, argtypes):
        import ctypes

        def recorded(*args):
            ranges = self._ranges() if self.eng is not None else {}
            words = [symbol[3:]]
            for a, ty in zip(args, argtypes):
                if ty is ctypes.c_void_p:
                    words.append(self.pointer(a, ranges))
                else:
                    words.append(repr(float(a)) if ty is ctypes.c_float else str(int(a)))
            self.lines.append(" ".join(words))
            return fn(*args)

        return recorded


def install(monkeypatch, decode_file=None):
    """-> (the decode module under trace, the recorder)."""
    import _fake_abi as F
    import qserve_amd.backend._util as U
    from qserve_amd._lib import SIGNATURES, lib
    F.install(monkeypatch)
    mods = [importlib.import_module("qserve_amd." + m)
            for m in ("append", "sampling", "penalties", "drafting", "stopping", "logprobs", "constraints", "lora")]
    if decode_file is None:
        D = importlib.import_module("qserve_amd.decode")
    else:
        spec = importlib.util.spec_from_file_location("qserve_amd._decode_under_trace", decode_file)
        D = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(D)
        mods.append(D)
    for m in mods:
        for attr in ("stream", "expect", "guard"):
            if hasattr(m, attr):
                monkeypatch.setattr(m, attr, getattr(U, attr))
    rec = Recorder()
    rec.monkeypatch = monkeypatch
    for symbol, (_, argtypes) in SIGNATURES.items():
        fn = F.SYMBOLS.get(symbol) or STEERING.get(symbol) or (lambda *a: 0)
        monkeypatch.setattr(lib, symbol, rec.wrap(symbol, fn, argtypes), raising=True)
    return D, rec


# ---- the scenarios -----------------------------------------------------------------------------------------------------------------
def _engine(D, rec, cfg=None, batch=2, prompt_len=5, max_new=4, **kw):
    return rec.watch(D.DecodeEngine(cfg or D.TINY, batch, prompt_len, max_new, device="cpu", seed=3, **kw))


def _prefill_two_steps(D, rec, **kw):
    eng = _engine(D, rec, **kw)
    eng.prefill(5)
    eng.step()
    eng.step()


def _planes(D, rec):
    cfg = dict(D.TINY, hidden=2048, heads=16, kv_heads=4, inter=2048, layers=2, vocab=256)
    eng = _engine(D, rec, cfg=cfg, prompt_len=3, planes=("down", "o"))
    assert set(eng.planes) == {"down", "o"}
    eng.prefill(3)
    eng.step()
    eng.step()


def _tp_rank(D, rec):
    eng = _engine(D, rec, tp_rank=1, tp_world=2)
    assert eng.vocab_parallel
    eng.prefill(5)
    for _ in range(2):
        for partial in eng._segments():
            rec.lines.append("yield " + rec.pointer(partial.data_ptr(), rec._ranges()) + f" {partial.numel()}")


def _chunked(D, rec):
    _engine(D, rec, prompt_len=7).prefill_chunked(7, 3)                  # chunks of 3, 3 and 1 tokens


def _shared(D, rec):
    eng = _engine(D, rec, prompt_len=110)                                # P = 70: one whole page, 6 tokens beyond it; R = 6 + 40
    g = torch.Generator().manual_seed(2)
    eng.prefill_shared(torch.randint(0, 512, (70,), generator=g), torch.randint(0, 512, (2, 40), generator=g), chunk=32)


def _verify(D, rec, device_walk):
    eng = _engine(D, rec)
    eng.prefill(5)
    eng.verify_tree(torch.zeros((2, len(PAR)), dtype=torch.int64), PAR, device_walk=device_walk)


def _sampled_penalised(D, rec):
    eng = _engine(D, rec, max_new=40)
    toks = torch.randint(0, 512, (2 * 5,), generator=torch.Generator().manual_seed(1))
    eng.prefill(5, toks)
    eng.enable_drafting(toks, max_ngram=3, min_match=1, pad_token=7)
    eng.set_sampling(0.8, top_k=5, top_p=0.9, seed=11)
    eng.set_penalties(1.2, 0.1, 0.1)
    eng.step()
    eng.verify_tree(torch.zeros((2, len(PAR)), dtype=torch.int64), PAR, device_walk=True, sampled=True)
    eng.speculate(PAR, sampled=True)


def _sampled_prefill(D, rec):
    eng = _engine(D, rec)
    eng.set_sampling(0.8, top_k=5, top_p=0.9, seed=11)
    eng.prefill(5)
    eng.step()
    eng.verify_tree(torch.zeros((2, len(PAR)), dtype=torch.int64), PAR, sampled=True)


def _dfa():
    """Four token classes (token % 4), three states; every state allows two of the classes."""
    from qserve_amd.constraints import TokenDFA
    nxt = [[(s + c) % 3 if (s + c) % 2 else -1 for c in range(4)] for s in range(3)]
    return TokenDFA((torch.arange(512) % 4).to(torch.int16), torch.tensor(nxt, dtype=torch.int32))


def _featured_engine(D, rec, stopping=False, logprobs=False, constraint=None, sampled=False):
    """A drafting engine behind its prefill with the features switched on where each may be: the constraint (start states [0, -1]),
    log-probabilities and sampling in front of the prefill - the prompt head masks, records and advances -, penalties and stopping
    behind enable_drafting (set_stopping looks at the current token: the `check_root` call)."""
    eng = _engine(D, rec, max_new=40)
    toks = torch.randint(0, 512, (2 * 5,), generator=torch.Generator().manual_seed(1))
    if sampled:
        eng.set_sampling(0.8, top_k=5, top_p=0.9, seed=11)
    if logprobs:
        eng.set_logprobs(top=3)
    if constraint is not None:
        eng.set_constraint(constraint, [0, -1])
    eng.prefill(5, toks)
    eng.enable_drafting(toks, max_ngram=3, min_match=1, pad_token=7)
    if sampled:
        eng.set_penalties(1.2, 0.1, 0.1)
    if stopping:
        eng.set_stopping(stop=[3, [4, 5]], max_new_tokens=[6, 30])
    return eng


def _featured(D, rec, stopping=False, logprobs=False, constraint=False, sampled=False):
    eng = _featured_engine(D, rec, stopping, logprobs, _dfa() if constraint else None, sampled)
    eng.step()
    eng.verify_tree(torch.zeros((2, len(PAR)), dtype=torch.int64), PAR, device_walk=True, sampled=sampled)
    eng.speculate(PAR, sampled=sampled)


class _Replay:
    def __init__(self, fn):
        self.replay = fn


def _generate(D, rec):
    """generate() over the stand-in for `_capture`: a `capture` line wherever the engine finds its graph missing or stale - and none
    where it must not."""
    dfa, other = _dfa(), _dfa()
    eng = _featured_engine(D, rec, stopping=True, logprobs=True, constraint=dfa)

    def capture(fn, advance):
        rec.lines.append("capture")
        res = fn()
        eng._len_bound -= advance
        return _Replay(fn), res

    def captures(n, *args, **kw):
        before = rec.lines.count("capture")
        rec.lines.append("generate " + " ".join([*map(str, args), *(f"{k}={v}" for k, v in kw.items())]))
        eng.generate(*args, **kw)
        assert rec.lines.count("capture") - before == n, f"generate{args, kw}: {rec.lines.count('capture') - before} captures, not {n}"

    eng._capture = capture
    captures(1, 3, poll_every=2)                                         # no step graph yet
    eng.set_logprobs(None)
    captures(1, 1)                                                       # another state of set_logprobs
    captures(1, 2, parents=PAR)                                          # no speculate graph yet
    captures(0, 1, parents=PAR)
    eng.set_constraint(dfa, [0, -1])                                     # the same automaton, new states: the tables stay
    captures(0, 1)
    captures(0, 1, parents=PAR)
    eng.set_constraint(other, [0, -1])                                   # another automaton: other tables
    captures(1, 1)
    captures(1, 1, parents=PAR)
    eng.set_constraint(None)                                             # off and back with no capture in between: the tables stay
    eng.set_constraint(other, [0, -1])
    captures(0, 1)
    captures(0, 1, parents=PAR)
    captures(1, 1, parents=[-1, 0, 1])                                   # another tree
    eng.set_sampling(0.8, top_k=5, top_p=0.9, seed=11)
    captures(1, 1, parents=[-1, 0, 1], sampled=True)                     # another head
    captures(0, 1, parents=[-1, 0, 1], sampled=True)


def _lora_seam(D, rec):
    """Record the `lora_rows` calls at the Python seam."""
    def lora_rows(out, x, x_scale, A, B, scaling, seq_adapter, rows_per_seq, seg_ends, workspace=None):
        ranges = rec._ranges()
        rec.lines.append("lora_rows " + " ".join(rec.pointer(t.data_ptr(), ranges) for t in (out, x, workspace)) + f" {rows_per_seq}")

    rec.monkeypatch.setattr(D.loramod, "lora_rows", lora_rows)


def _lora(D, rec):
    """The `lora_rows` calls of a prefill, a step and a device-walk verification, at the Python seam."""
    _lora_seam(D, rec)
    eng = _engine(D, rec)
    eng.enable_lora(2, 8)
    eng.set_lora([0, -1])
    eng.prefill(5)
    eng.step()
    eng.verify_tree(torch.zeros((2, len(PAR)), dtype=torch.int64), PAR, device_walk=True)


def _pool_stand_ins(rec):
    """The page entries on the host: the stand-ins of tests/test_page_pool_contracts.py under the recorder, `paging` on the host seams."""
    import qserve_amd.backend._util as U
    import test_page_pool_contracts as C
    from qserve_amd import paging
    from qserve_amd._lib import SIGNATURES, lib
    for attr in ("stream", "expect", "guard"):
        rec.monkeypatch.setattr(paging, attr, getattr(U, attr))
    for symbol, fn in (("qs_pages_reserve", C._fake_reserve), ("qs_pages_release", C._fake_release)):
        rec.monkeypatch.setattr(lib, symbol, rec.wrap(symbol, fn, SIGNATURES[symbol][1]))


def _admit_prompts():
    g = torch.Generator().manual_seed(4)
    return [torch.randint(0, 512, (n,), generator=g) for n in (3, 9)]


def _admit(D, rec, featured=False):
    """One ragged admit into rows [2, 0] of an empty batch of three: prompts of 3 and 9 tokens in passes of 4 - three passes, the short
    sequence leaves after the first.  `featured`: under a page pool with sampling, log-probabilities, a constraint, penalties and
    stopping all on - the admission head does not penalise -, and one step() behind it."""
    if featured:
        _pool_stand_ins(rec)
    eng = _engine(D, rec, batch=3, prompt_len=9, max_new=4, page_pool=5 if featured else None)
    eng.enable_drafting(None, max_ngram=3, min_match=1, pad_token=7)
    if featured:
        eng.set_sampling(0.8, top_k=5, top_p=0.9, seed=11)
        eng.set_logprobs(top=3)
        eng.set_constraint(_dfa(), [0, -1, 1])
        eng.set_penalties(1.2, 0.1, 0.1)
    eng.set_stopping([3], 0)
    at = len(rec.lines)
    eng.admit([2, 0], _admit_prompts(), max_new_tokens=[2, 3], text_start=[2, 9], chunk=4, **(dict(start_states=[1, 0]) if featured else {}))
    assert not any(line.startswith("penalize_rows") for line in rec.lines[at:])
    if featured:
        eng.step()
        assert any(line.startswith("penalize_rows") for line in rec.lines[at:])


def _admit_lora(D, rec):
    """The `lora_rows` calls of a ragged admit (9 and 3 tokens in passes of 4) under per-sequence adapters: one id per token."""
    _lora_seam(D, rec)
    eng = _engine(D, rec, batch=3, prompt_len=9, max_new=4)
    eng.enable_lora(2, 8)
    eng.enable_drafting(None)
    eng.set_lora([0, 1, -1])
    eng.admit([1, 0], _admit_prompts()[::-1], chunk=4)


SCENARIOS = {
    "per_channel_fused": lambda D, rec: _prefill_two_steps(D, rec, group_size=-1, fuse_pairs=True),
    "per_channel_op_by_op": lambda D, rec: _prefill_two_steps(D, rec, group_size=-1, fuse_pairs=False),
    "per_group_fused": lambda D, rec: _prefill_two_steps(D, rec, group_size=128, fuse_pairs=True),
    "per_group_op_by_op": lambda D, rec: _prefill_two_steps(D, rec, group_size=128, fuse_pairs=False),
    "planes_down_o": _planes,
    "qkv_bias": lambda D, rec: _prefill_two_steps(D, rec, cfg=dict(D.TINY, qkv_bias=True)),
    "tp2_rank1_segments": _tp_rank,
    "prefill_chunked_ragged": _chunked,
    "prefill_shared_chunked": _shared,
    "verify_tree_host_walk": lambda D, rec: _verify(D, rec, False),
    "verify_tree_device_walk": lambda D, rec: _verify(D, rec, True),
    "sampled_penalised_step_verify_speculate": _sampled_penalised,
    "sampled_prefill_step_host_verify": _sampled_prefill,
    "stopping_step_verify_speculate": lambda D, rec: _featured(D, rec, stopping=True),
    "logprobs_step_verify_speculate": lambda D, rec: _featured(D, rec, logprobs=True),
    "constraint_step_verify_speculate": lambda D, rec: _featured(D, rec, constraint=True),
    "stopping_logprobs_constraint": lambda D, rec: _featured(D, rec, stopping=True, logprobs=True, constraint=True),
    "stopping_logprobs_constraint_sampled_penalised": lambda D, rec: _featured(D, rec, True, True, True, sampled=True),
    "generate_recaptures": _generate,
    "lora_prefill_step_verify": _lora,
    "admit_ragged": _admit,
    "admit_pooled_featured": lambda D, rec: _admit(D, rec, featured=True),
    "admit_lora": _admit_lora,
}


def trace(name, monkeypatch, decode_file=None):
    D, rec = install(monkeypatch, decode_file)
    with np.errstate(all="ignore"):                                      # (the attention stubs leave their outputs unwritten)
        SCENARIOS[name](D, rec)
    return rec.lines


def _golden():
    with open(GOLDEN) as f:
        g = json.load(f)
    return {name: [g["lines"][i] for i in idx] for name, idx in g["traces"].items()}


def test_the_golden_covers_every_scenario_and_stays_small():
    assert sorted(_golden()) == sorted(SCENARIOS)
    assert os.path.getsize(GOLDEN) <= MAX_GOLDEN_BYTES


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_engine_issues_the_recorded_calls(built_lib, monkeypatch, name):
    want, got = _golden()[name], trace(name, monkeypatch)
    for i, (w, g) in enumerate(zip(want, got)):
        assert g == w, f"{name}: call {i} differs\n  recorded: {w}\n  issued:   {g}\n  after:    {got[max(0, i - 3):i]}"
    assert len(got) == len(want), f"{name}: {len(got)} calls issued, {len(want)} recorded; the first beyond: {(got + want)[min(len(got), len(want))]}"


def _record(decode_file):
    table, traces = {}, {}
    for name in SCENARIOS:
        mp = pytest.MonkeyPatch()
        try:
            traces[name] = [table.setdefault(line, len(table)) for line in trace(name, mp, decode_file)]
        finally:
            mp.undo()
    with open(GOLDEN, "w") as f:
        f.write('{"lines":[\n' + ",\n".join(json.dumps(line) for line in table) + '\n],"traces":{\n')
        f.write(",\n".join(f'{json.dumps(name)}:{json.dumps(idx, separators=(",", ":"))}' for name, idx in traces.items()) + "\n}}\n")
    print(f"{GOLDEN}: {len(table)} distinct lines, {sum(map(len, traces.values()))} calls, {os.path.getsize(GOLDEN)} bytes")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", action="store_true", required=True)
    ap.add_argument("--decode", default=None, help="another revision of qserve_amd/decode.py to record from")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    from qserve_amd import build
    build.build(verbose=False)
    _record(args.decode)
