"""One tree verification of DecodeEngine three ways, in ONE run: the host path (verify_tree as it was: two read-backs, the walk in
Python, one commit_path per layer), the device walk run eagerly (verify_tree(device_walk=True)) and the captured replay
(capture_verify / run_verify).  Llama-3-8B shapes, KV4, synthetic weights, a cache of 1 024 tokens per sequence:

    B in {1, 8}  x  a 16-node and a 64-node tree (random forests off one root), random drafts

Every timed call starts from the same state (root tokens, lengths = 1 025: restored outside the timed window), is timed with a host clock
around the call AND a device synchronise (the host path's own read-backs are part of what it costs), after warm-up calls of the same
shape; the figure is the median of --iters calls, and every variant is measured --reps times in alternation so that the spread between
repeated medians of the same thing is known.  Next to the times: the calls of the library's C entries one verification makes (counted
in a call of its own, not a timed one) - each is one kernel launch, split-KV attention two.  Run it under `timeout`.

    python scripts/bench_verify_tree.py [--iters 20] [--warmup 3] [--reps 3] [--out profiles/verify_tree_device.txt]
"""
import argparse
import collections
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PAST = 1024
TREES = (16, 64)
BATCHES = (1, 8)


class count_library_calls:
    """Counts the calls of every C entry of the library while active (the Python layers look the entries up per call)."""

    def __enter__(self):
        from qserve_amd._lib import SIGNATURES, lib
        self.lib, self.saved, self.calls = lib, {}, collections.Counter()
        for name in SIGNATURES:
            fn = getattr(lib, name, None)
            if fn is None:
                continue
            self.saved[name] = fn

            def counted(*a, _fn=fn, _name=name):
                self.calls[_name] += 1
                return _fn(*a)

            setattr(lib, name, counted)
        return self

    def __exit__(self, *exc):
        for name, fn in self.saved.items():
            setattr(self.lib, name, fn)
        return False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    assert a.iters >= 10 and a.reps >= 2
    assert torch.cuda.is_available(), "bench_verify_tree needs a GPU"
    from qserve_amd.decode import LLAMA3_8B, DecodeEngine
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"# {torch.cuda.get_device_name(0)}; {LLAMA3_8B['name']} shapes, KV4, synthetic weights, past {PAST}; one verification, host clock around "
        f"call + device synchronise, ms; median of {a.iters} calls, {a.reps} such medians per variant in alternation: lowest .. highest")
    summary = []
    for B in BATCHES:
        eng = DecodeEngine(LLAMA3_8B, batch=B, prompt_len=PAST, max_new=128, device="cuda:0", seed=0)
        eng.prefill_cache(PAST)                                  # lengths = PAST + 1: the tree sits on a past of PAST tokens

        tok0 = eng.tokens.clone()

        def reset():
            eng.tokens.copy_(tok0)
            eng.lengths.fill_(PAST + 1)
            eng._len_bound = PAST + 1

        for n in TREES:
            par = [-1] + [int(rng.integers(0, i)) for i in range(1, n)]
            drafts = [torch.from_numpy(rng.integers(0, LLAMA3_8B["vocab"], size=(B, n))).to(dev) for _ in range(4)]
            reset()
            eng.capture_verify(par, max_past=PAST)               # (the hint the eager calls below give: the plans are the same)
            variants = {
                "host path": lambda d: eng.verify_tree(d, par),
                "device walk, eager": lambda d: eng.verify_tree(d, par, device_walk=True),
                "device walk, captured": lambda d: eng.run_verify(d),
            }
            # the three agree on the same state and draft (checked before anything is timed), and what each one calls
            results, calls = {}, {}
            for k, fn in variants.items():
                reset()
                torch.cuda.synchronize()
                with count_library_calls() as c:
                    r = fn(drafts[0])
                    torch.cuda.synchronize()
                results[k] = [x.clone() for x in r] + [eng.tokens.clone(), eng.lengths.clone()]
                calls[k] = c.calls
            for k in list(variants)[1:]:
                assert all(torch.equal(x, y) for x, y in zip(results["host path"], results[k])), f"{k} differs from the host path"

            def median_ms(fn):
                ts = []
                for i in range(a.warmup + a.iters):
                    reset()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn(drafts[i % len(drafts)])
                    torch.cuda.synchronize()
                    ts.append((time.perf_counter() - t0) * 1e3)
                return statistics.median(ts[a.warmup:])

            meds = {k: [] for k in variants}
            for _ in range(a.reps):
                for k, fn in variants.items():
                    meds[k].append(median_ms(fn))
            say(f"\nB={B} n={n}:")
            for k, v in meds.items():
                c = calls[k]
                say(f"    {k:24s} {min(v):8.3f} .. {max(v):8.3f} ms   library calls {sum(c.values()):4d} (commit_path {c['qs_kv_cache_commit_path']}, "
                    f"commit_path_layers {c['qs_kv_cache_commit_path_layers']}, tree_accept_greedy {c['qs_tree_accept_greedy']})")
            say("    (host path: 2 device read-backs + host-built index tensors; device walk: none; captured: 1 copy of the drafts + 1 graph launch,"
                " its library calls were made once, at capture)")
            t = {k: statistics.median(v) for k, v in meds.items()}
            spread = max(max(v) - min(v) for v in meds.values())
            summary.append(f"    B={B:<2d} n={n:<3d}: host {t['host path']:8.3f} ms, device walk eager {t['device walk, eager']:8.3f} ms (x{t['device walk, eager'] / t['host path']:5.3f}), "
                           f"captured {t['device walk, captured']:8.3f} ms (x{t['device walk, captured'] / t['host path']:5.3f}); largest spread {spread:6.3f} ms")
        del eng
        torch.cuda.empty_cache()
    say("\n# summary: medians of the medians, and each device-walk variant as a multiple of the host path (below 1 = faster)")
    for s in summary:
        say(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
