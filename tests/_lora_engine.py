"""Engines under LoRA adapters shared by tests/test_lora_engine_gpu.py - and, run as a program, the body of its capture test, which
starts this file in a fresh Python process because a failed capture leaves the HIP context unusable and nothing else may
share it.

Setting of tests/_accept_engine.py / tests/_speculate_engine.py: TINY, B = 3, P = 70, seed 5, the 12-node tree PAR.  The table holds two
slots of rank 16: slot 0 an adapter of rank 8 (zero-padded) with alpha 32, slot 1 one of rank 16 with alpha 24, both over all seven
modules of both layers, large enough to change what the model says."""
import os
import sys

import torch

import _accept_engine as E
import _speculate_engine as S
from _lora_cases import peft_adapter

SLOTS, RANK = 2, 16
MIXED = [0, 1, -1]
STD = 0.05


def load_adapters(e):
    from qserve_amd.decode import TINY
    e.load_lora(0, peft_adapter(TINY, 8, seed=11, std=STD), alpha=32)
    e.load_lora(1, peft_adapter(TINY, 16, seed=12, std=STD), alpha=24)


def lora_engine(toks, ids, chunk=None, drafting=False):
    """An engine whose prompt already ran under the adapters `ids`: enable_lora, the two adapters, set_lora, then prefill (in chunks of
    `chunk` tokens where given), then drafting where asked for."""
    from qserve_amd.decode import TINY, DecodeEngine
    e = DecodeEngine(TINY, batch=E.B, prompt_len=E.P, max_new=40, device="cuda:0", seed=5)
    e.enable_lora(SLOTS, RANK)
    load_adapters(e)
    e.set_lora(ids)
    if chunk is None:
        e.prefill(E.P, toks)
    else:
        e.prefill_chunked(E.P, chunk, toks)
    if drafting:
        e.enable_drafting(toks, **S.NGRAM)
    return e


def capture_main():
    """A captured step and a captured speculate round with LoRA on against their eager twins over three replays each; then set_lora with
    other ids under the captured graphs - no re-capture - and one more replay of each against the twin with the same change."""
    gpu = torch.device("cuda:0")
    toks = E.prompt(gpu)
    # ---- the step
    cap, twin = lora_engine(toks, MIXED), lora_engine(toks, MIXED)
    cap.capture()                                            # (its warm-up is a real step)
    twin.step()
    assert cap._step_capture.state["lora"] is True and cap._step_capture.keep[1]["lora"] is not None
    E.assert_same_state(cap, twin, "after capture")
    graph = cap.graph
    for i in range(4):
        if i == 3:
            for e in (cap, twin):
                e.set_lora([1, -1, 0])
            assert cap.graph is graph
        cap.run()
        twin.step()
        E.assert_same_state(cap, twin, f"step replay {i}")
    base = lora_engine(toks, [-1, -1, -1])
    for _ in range(5):
        base.step()
    torch.cuda.synchronize()
    assert not torch.equal(base.hidden, cap.hidden), "five steps under adapters left the hidden rows of the base model"
    print(f"step: tokens {cap.tokens.tolist()}, base model {base.tokens.tolist()}")
    # ---- the speculate round
    cap, twin, ref = (lora_engine(toks, MIXED, drafting=True) for _ in range(3))
    cap.capture_speculate(E.PAR)
    twin.speculate(E.PAR)
    ref.speculate(E.PAR)
    assert cap._speculate_capture.state["lora"] is True
    E.assert_same_state(cap, twin, "after capture_speculate")
    S.plant(ref, (cap, twin))                                # (ref runs under the same adapters: what it says next is what the twins will say)
    graph, longest = cap.speculate_graph, 0
    for i in range(4):
        if i == 3:
            for e in (cap, twin):
                e.set_lora([1, -1, 0])
            assert cap.speculate_graph is graph
        got = cap.run_speculate()
        want = twin.speculate(E.PAR)
        torch.cuda.synchronize()
        E.assert_same_result(got, want, f"round replay {i}")
        E.assert_same_state(cap, twin, f"round replay {i}")
        S.assert_same_text(cap, twin, f"round replay {i}")
        longest = max(longest, int(got[1].max()))
        print(f"round replay {i}: accepted path lengths {got[1].tolist()}")
    assert longest >= 2, "the planted continuation was accepted nowhere: the replays checked root-only paths"
    print("LORA-CAPTURE-OK")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    {"capture": capture_main}[sys.argv[1]]()
