"""What the stop rule of DecodeEngine.set_stopping costs, in ONE run (no pass / fail threshold; figures only), at the bench configuration:
Llama-3-8B shapes, KV4, synthetic weights, B = 64, prompt 1 024.

  1. per captured step(): the step graph captured with stopping off and the one captured with stopping on (an empty table and no
     limit below the history's capacity: no sequence ever stops, so both do the same model work), over the same engine, from the same
     restored state.  Host clock around --replays replays + device synchronise, per-replay mean; --reps such figures per graph in
     alternation; the medians and the median of the pairwise differences.
  2. per captured speculate round (a 16-node tree): the same with capture_speculate.
  3. generate(rounds, poll_every=8) - one read-back of (finished, lengths) per 8 rounds - against a loop that replays the same graph
     and reads `tokens` back after every round, what a host-side stop check needs.

Run it under `timeout`.

    python scripts/bench_stop_update.py [--replays 50] [--reps 9] [--rounds 64] [--out profiles/stop_update.txt]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PROMPT, BATCH, MAX_NEW = 1024, 64, 640


def deep_tree(n, width=2):
    """A chain with `width` - 1 extra leaves per level (scripts/bench_speculate.py's tree)."""
    par, spine = [-1], 0
    while len(par) < n:
        first = len(par)
        for _ in range(width):
            if len(par) < n:
                par.append(spine)
        spine = first
    return par


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--rounds", type=int, default=64)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    assert a.replays >= 10 and a.reps >= 3 and 8 <= a.rounds <= MAX_NEW // 2
    assert torch.cuda.is_available(), "bench_stop_update needs a GPU"
    from qserve_amd.decode import LLAMA3_8B, DecodeEngine
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"# {torch.cuda.get_device_name(0)}; {LLAMA3_8B['name']} shapes, KV4, B = {BATCH}, prompt {PROMPT}; stop table [32, 8], no sequence ever stops")
    prompt = torch.randint(0, LLAMA3_8B["vocab"], (BATCH * PROMPT,), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    eng = DecodeEngine(LLAMA3_8B, batch=BATCH, prompt_len=PROMPT, max_new=MAX_NEW, device="cuda:0", seed=0)
    eng.prefill_chunked(PROMPT, 256, prompt)
    eng.enable_drafting(prompt)
    state0 = (eng.tokens.clone(), eng.lengths.clone(), eng.history.clone(), eng.hidden.clone())

    def reset():
        """tokens, lengths and the text as after the prefill (the cache behind the lengths is overwritten by whoever runs next)."""
        eng.tokens.copy_(state0[0])
        eng.lengths.copy_(state0[1])
        eng.history.copy_(state0[2])
        eng.hidden.copy_(state0[3])
        eng._len_bound = PROMPT + 1

    par = deep_tree(16)
    graphs = {}
    eng.capture()                                            # stopping off: what every path launches today
    graphs["step", "off"] = eng.graph
    reset()
    eng.capture_speculate(par)
    graphs["round", "off"] = eng.speculate_graph
    reset()
    eng.set_stopping([], None)                               # on, and nothing ever stops
    eng.capture()
    graphs["step", "on"] = eng.graph
    reset()
    eng.capture_speculate(par)
    graphs["round", "on"] = eng.speculate_graph
    reset()

    def per_replay_us(g, n):
        reset()
        for _ in range(3):
            g.replay()
        reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            g.replay()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / n

    say(f"\n# 1. / 2. host clock around {a.replays} step replays ({max(a.replays // 4, 10)} round replays) + device synchronise, us per replay; "
        f"{a.reps} figures per graph in alternation")
    for what, n in (("step", a.replays), ("round", max(a.replays // 4, 10))):
        off, on = [], []
        for _ in range(a.reps):
            off.append(per_replay_us(graphs[what, "off"], n))
            on.append(per_replay_us(graphs[what, "on"], n))
        diffs = [y - x for x, y in zip(off, on)]
        say(f"    captured {what:5s} stopping off {statistics.median(off):9.1f} us ({min(off):.1f} .. {max(off):.1f})   on {statistics.median(on):9.1f} us "
            f"({min(on):.1f} .. {max(on):.1f})   on - off: median of pairs {statistics.median(diffs):+7.2f} us ({min(diffs):+.2f} .. {max(diffs):+.2f})")
    assert int(eng.finished.sum()) == 0, "a sequence stopped: the two graphs did not do the same work"

    say(f"\n# 3. {a.rounds} rounds of the captured step graph (stopping on): generate(poll_every=8) against a loop that reads `tokens` back every "
        f"round; ms for the {a.rounds} rounds, {a.reps} figures each in alternation")

    def generate_ms():
        reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, _, rounds, reads = eng.generate(a.rounds, poll_every=8)
        dt = (time.perf_counter() - t0) * 1e3
        assert rounds == a.rounds and reads == -(-a.rounds // 8)
        return dt

    def readback_ms():
        reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.rounds):
            eng.run()
            eng.tokens.cpu()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    gen, rb = [], []
    for i in range(1 + a.reps):                              # (the first pair is the warm-up)
        gen.append(generate_ms())
        rb.append(readback_ms())
    gen, rb = gen[1:], rb[1:]
    say(f"    generate()            {statistics.median(gen):9.2f} ms ({min(gen):.2f} .. {max(gen):.2f})   [includes reading the texts back once at the end]")
    say(f"    read back every round {statistics.median(rb):9.2f} ms ({min(rb):.2f} .. {max(rb):.2f})")
    say(f"    per round: {statistics.median(gen) * 1e3 / a.rounds:.1f} us against {statistics.median(rb) * 1e3 / a.rounds:.1f} us")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
