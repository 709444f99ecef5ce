"""Expected values of the greedy walk over a verified draft tree (qs_tree_accept_greedy, DecodeEngine.verify_tree): the rule in plain
Python, and the random cases the CPU and the GPU tests share.

The rule, for one sequence of n nodes (`parents[i]`: an index into the sequence, -1 = hangs off the context; `tokens[i]`: the token node i
carries; `argmax[i]`: the model's arg-max at node i): node 0 is accepted; from the current node `cur` the next one is the lowest c with
cur < c < n, parents[c] == cur and tokens[c] == argmax[cur]; the walk ends when there is none or the path holds `cap` nodes."""
from _tree_cases import random_parents

MAX_NODES = 64


def reference_walk(parents, tokens, argmax, cap):
    """-> the accepted path (node indices, strictly increasing; [] for an empty sequence).  Nodes beyond 64 are ignored."""
    n = min(len(parents), MAX_NODES)
    if n == 0:
        return []
    path, cur = [0], 0
    while len(path) < cap:
        nxt = next((c for c in range(cur + 1, n) if parents[c] == cur and tokens[c] == argmax[cur]), None)
        if nxt is None:
            break
        path.append(nxt)
        cur = nxt
    return path


def random_case(rng, n, vocab):
    """(parents, tokens, argmax) of one n-node tree with a single root: a small `vocab` makes matches - and sibling ties - frequent."""
    parents = random_parents(rng, n, roots=0.0)
    tokens = [int(x) for x in rng.integers(0, vocab, size=n)]
    argmax = [int(x) for x in rng.integers(0, vocab, size=n)]
    return parents, tokens, argmax


def random_cases(seed=11, n=24, vocab=3, count=200):
    """The shared set: tests/test_tree_accept_cpu.py pins its path-length mix, tests/test_tree_accept_gpu.py runs the kernel on it."""
    import numpy as np
    rng = np.random.default_rng(seed)
    return [random_case(rng, n, vocab) for _ in range(count)]


# parents no tree has: later nodes, self-loops, values below -1, indices beyond the sequence (tokens = argmax = 0 everywhere, so
# every edge the rule can follow is followed)
MALFORMED = [
    [-1, 2, 1, 3, 5, 4],                 # a later node / a 2-cycle
    [0, 1, 2, 3],                        # every node its own parent (node 0 included)
    [-1, 0, -7, 2, 1 << 30, -(1 << 31)],  # far out of range on both sides
    [5, 0, 0, 1, 1, 0],                  # the root hangs off a later node
    [-1] + [63 - i for i in range(63)],  # n = 64, parents run backwards
    [-1, 0, 1, 1, 3, 3, 3, 64, 65, 7],   # indices >= n
]


def host_loop(par, tokens, argmax):
    """The loop of DecodeEngine.verify_tree's host path, verbatim (one sequence): children lists, first matching child."""
    n = len(par)
    kids = [[c for c in range(1, n) if par[c] == i] for i in range(n)]
    path, cur = [0], 0
    while True:
        nxt = next((c for c in kids[cur] if tokens[c] == argmax[cur]), None)
        if nxt is None:
            break
        path.append(nxt)
        cur = nxt
    return path
