"""What constrained decoding costs (`qs_constrain_rows`, DecodeEngine.set_constraint), in ONE run (no pass / fail threshold; figures only):

  1. the mask launch on 64 rows (a decode step at B = 64) and on 64 x 12 rows (a verification of a 12-node tree) of the Llama-3-8B
     vocabulary (n = 128 256), for C = 256 and C = 32 768 classes, at 10 % and 90 % allowed tokens - once on FRESH rows (every launch of
     the timed batch gets a copy of its own that no launch has masked yet: the stores happen) and once on rows that are masked already
     (nothing changes, nothing is stored) - next to `qs_penalize_rows` (a history of 1 024 tokens) and `qs_argmax_rows` on the same
     rows in the same run, as the yardsticks: the launch the mask sits behind and the one it sits in front of;
  1b. the mask launch at C = 32 768 under three class layouts of the vocabulary - uniformly random classes (what 1. uses), contiguous
     runs of ids per class, and a layout that sends every mask read of a wave to one LDS bank (the worst there is);
  2. the captured Llama-3-8B step at B = 64 (KV4, prompt 1 024) with the constraint off, on with every state -1 (the launches exist, every
     workgroup leaves at once) and on with every sequence constrained (C = 256, 64 states, half of the classes allowed), as an
     in-process A/B: the three graphs replayed in alternation.

Part 1: HIP events around --iters back-to-back launches after warm-up launches of the same shape, per-launch times of --reps such
batches per variant in alternation: lowest .. highest, medians in the summary.  Part 2: a host clock around --replays replays that end
in a device synchronise.  Run it under `timeout`.

    python scripts/bench_constrain_rows.py [--iters 20] [--warmup 3] [--reps 5] [--replays 50] [--skip-step] [--only-layouts] [--out profiles/constrain_rows.txt]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N, STATES = 128256, 64
ROWS = (64, 64 * 12)
CLASSES = (256, 32768)
ALLOWED = (0.1, 0.9)
LAYOUT_C, LAYOUT_STRIDE = 32768, 2048                     # 1b: classes LAYOUT_STRIDE apart have their mask words 64 words apart
PROMPT, BATCH, MAX_NEW = 1024, 64, 640


def random_tables(C, allowed, dev, gen):
    """token_class uniform over the classes; next: a fraction `allowed` of every state's classes goes on to a random state."""
    token_class = torch.randint(0, C, (N,), device=dev, generator=gen).to(torch.int16)
    nxt = torch.randint(0, STATES, (STATES, C), device=dev, generator=gen, dtype=torch.int32)
    nxt[torch.rand((STATES, C), device=dev, generator=gen) >= allowed] = -1
    nxt[:, 0] = torch.arange(STATES, device=dev, dtype=torch.int32)       # (no state without a way on)
    return token_class, nxt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--skip-step", action="store_true", help="part 1 only (no 8B engine)")
    ap.add_argument("--only-layouts", action="store_true", help="part 1b only")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    assert a.iters >= 10 and a.reps >= 3 and a.replays >= 10
    assert torch.cuda.is_available(), "bench_constrain_rows needs a GPU"
    from qserve_amd.constraints import TokenDFA, constrain_rows
    from qserve_amd.decode import argmax_rows_
    from qserve_amd.penalties import penalize_rows
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def timed_us(fns):
        """HIP events around the calls of `fns`, back to back -> mean us per call."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for fn in fns:
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / len(fns)

    say(f"# {torch.cuda.get_device_name(0)}; 1. fp16 logits [rows, {N}] (standard normal x 3), {STATES} states, row states uniform over them; HIP "
        f"events around {a.iters} back-to-back launches, mean us per launch; {a.reps} such figures per variant in alternation: lowest .. highest")
    summary = []
    for rows in (() if a.only_layouts else ROWS):
        gen = torch.Generator(device=dev).manual_seed(rows)
        master = (torch.randn((rows, N), device=dev, generator=gen) * 3.0).half()
        pool = torch.empty((a.warmup + a.iters, rows, N), dtype=torch.float16, device=dev)
        row_state = torch.randint(0, STATES, (rows,), device=dev, generator=gen, dtype=torch.int32)
        out = torch.empty((rows,), dtype=torch.int64, device=dev)
        history = torch.randint(0, N, (rows, 1024), device=dev, generator=gen).int()
        lengths = torch.full((rows,), 1024, dtype=torch.int32, device=dev)
        for C in CLASSES:
            for allowed in ALLOWED:
                token_class, nxt = random_tables(C, allowed, dev, gen)

                def mask(i):
                    return lambda: constrain_rows(pool[i], row_state, token_class, nxt)

                def fresh():
                    pool.copy_(master.unsqueeze(0).expand_as(pool))
                    for i in range(a.warmup):
                        mask(i)()
                    return timed_us([mask(a.warmup + i) for i in range(a.iters)])

                def again(fn):
                    for _ in range(a.warmup):
                        fn()
                    return timed_us([fn] * a.iters)

                variants = {
                    "qs_constrain_rows, fresh rows": fresh,
                    "qs_constrain_rows, masked rows": lambda: again(mask(0)),
                    "qs_penalize_rows (history 1024)": lambda: again(lambda: penalize_rows(pool[1], history, lengths, None, None, None, 1.1, 0.01, 0.01)),
                    "qs_argmax_rows": lambda: again(lambda: argmax_rows_(pool[2], out)),
                }
                figs = {v: [] for v in variants}
                for _ in range(a.reps):
                    for v, fn in variants.items():
                        figs[v].append(fn())
                kept = float((pool[a.warmup] != float("-inf")).float().mean())
                say(f"\n  rows={rows} C={C} allowed={allowed:.0%} (finite logits left: {kept:.1%}):")
                for v, t in figs.items():
                    say(f"    {v:34s} {min(t):9.1f} .. {max(t):9.1f} us")
                t = {v: statistics.median(x) for v, x in figs.items()}
                f = t["qs_constrain_rows, fresh rows"]
                summary.append(f"    rows={rows:<4d} C={C:<6d} allowed={allowed:4.0%}: constrain_rows {f:8.1f} us fresh ({rows * N * 4 / f / 1e6:5.2f} TB/s of "
                               f"logit + class reads), {t['qs_constrain_rows, masked rows']:8.1f} us masked; x{f / t['qs_penalize_rows (history 1024)']:5.2f} of "
                               f"penalize_rows ({t['qs_penalize_rows (history 1024)']:8.1f} us), x{f / t['qs_argmax_rows']:5.2f} of argmax_rows "
                               f"({t['qs_argmax_rows']:8.1f} us)")
        del master, pool
        torch.cuda.empty_cache()
    if summary:
        say("\n# summary of 1.: medians; the fresh-row mask as bytes of logits and classes read per second and as a multiple of each yardstick")
        for s in summary:
            say(s)

    # the mask word a lane reads follows the class of its id, so LDS bank conflicts follow the class LAYOUT of the vocabulary
    say(f"\n# 1b. class layouts, C = {LAYOUT_C}, 50 % allowed, fresh rows, as in 1.: `uniform` (random classes, what 1. measures), `runs` (class = "
        f"id * C / n: neighbouring ids share a class, a lane's 8 ids read one word), `one bank` (class = {LAYOUT_STRIDE} * (id / 8 % {LAYOUT_C // LAYOUT_STRIDE}): "
        f"a lane's 8 ids share a class, {LAYOUT_C // LAYOUT_STRIDE} neighbouring lanes read {LAYOUT_C // LAYOUT_STRIDE} different mask words 64 words apart - every "
        f"read of a wave in one LDS bank, whether it has 32 or 64 of them, a {LAYOUT_C // LAYOUT_STRIDE}-way conflict)")
    for rows in ROWS:
        gen = torch.Generator(device=dev).manual_seed(1000 + rows)
        master = (torch.randn((rows, N), device=dev, generator=gen) * 3.0).half()
        pool = torch.empty((a.warmup + a.iters, rows, N), dtype=torch.float16, device=dev)
        row_state = torch.randint(0, STATES, (rows,), device=dev, generator=gen, dtype=torch.int32)
        uniform, nxt = random_tables(LAYOUT_C, 0.5, dev, gen)
        ids = torch.arange(N, device=dev)
        layouts = {"uniform": uniform, "runs": (ids * LAYOUT_C // N).to(torch.int16),
                   "one bank": (LAYOUT_STRIDE * (ids // 8 % (LAYOUT_C // LAYOUT_STRIDE))).to(torch.int16)}

        def fresh_layout(token_class):
            pool.copy_(master.unsqueeze(0).expand_as(pool))
            for i in range(a.warmup):
                constrain_rows(pool[i], row_state, token_class, nxt)
            return timed_us([(lambda i=i: constrain_rows(pool[a.warmup + i], row_state, token_class, nxt)) for i in range(a.iters)])

        figs = {v: [] for v in layouts}
        for _ in range(a.reps):
            for v, token_class in layouts.items():
                figs[v].append(fresh_layout(token_class))
        for v, t in figs.items():
            say(f"    rows={rows:<4d} {v:9s} {statistics.median(t):8.1f} us ({min(t):.1f} .. {max(t):.1f})")
        del master, pool
        torch.cuda.empty_cache()

    if not a.skip_step and not a.only_layouts:
        from qserve_amd.decode import LLAMA3_8B, DecodeEngine
        say(f"\n# 2. {LLAMA3_8B['name']} shapes, KV4, B = {BATCH}, prompt {PROMPT}: the captured step(), constraint off / on with every state -1 / on "
            f"with every sequence constrained (C = 256, {STATES} states, 50 % allowed); host clock around {a.replays} replays + device synchronise, us "
            f"per replay; {a.reps} figures per graph in alternation")
        prompt = torch.randint(0, LLAMA3_8B["vocab"], (BATCH * PROMPT,), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        eng = DecodeEngine(LLAMA3_8B, batch=BATCH, prompt_len=PROMPT, max_new=MAX_NEW, device="cuda:0", seed=0)
        eng.prefill_chunked(PROMPT, 256, prompt)
        state0 = (eng.tokens.clone(), eng.lengths.clone(), eng.hidden.clone())
        token_class, nxt = random_tables(256, 0.5, dev, torch.Generator(device=dev).manual_seed(2))
        dfa = TokenDFA(token_class.cpu(), nxt.cpu())
        starts = {"off": None, "on, states -1": [-1] * BATCH, "on, constrained": [b % STATES for b in range(BATCH)]}

        def reset(name):
            eng.tokens.copy_(state0[0])
            eng.lengths.copy_(state0[1])
            eng.hidden.copy_(state0[2])
            eng._len_bound = PROMPT + 1
            if starts[name] is not None:
                eng.set_constraint(dfa, starts[name])         # (the same automaton: the tables stay, the states are refilled in place)

        graphs = {}
        for name, st in starts.items():
            eng.set_constraint(None if st is None else dfa, 0)
            reset(name)
            eng.capture()
            graphs[name] = eng.graph

        def per_replay_us(name):
            g = graphs[name]
            reset(name)
            for _ in range(3):
                g.replay()
            reset(name)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.replays):
                g.replay()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e6 / a.replays

        figs = {name: [] for name in graphs}
        for _ in range(a.reps):
            for name in graphs:
                figs[name].append(per_replay_us(name))
        for name, t in figs.items():
            d = [y - x for x, y in zip(figs["off"], t)]
            say(f"    captured step, constraint {name:16s} {statistics.median(t):9.1f} us ({min(t):.1f} .. {max(t):.1f})   - off: median of pairs "
                f"{statistics.median(d):+7.2f} us ({min(d):+.2f} .. {max(d):+.2f})")
        say(f"    (states after the last constrained replays: {sorted(set(eng.fsm_state.tolist()))[:8]} ... - none dead: {-2 not in eng.fsm_state.tolist()})")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
