"""The device-side tail of tree verification without a GPU: the walk rule in plain Python (tests/_accept_cases.py) against the host loop
of DecodeEngine.verify_tree on hand-made trees, its termination on malformed parents, the path-length mix of the random cases the GPU
test runs the kernel on, and the refusals of the Python wrappers and of the two C entries (argument validation happens before any
device call, on made-up addresses)."""
import pytest
import torch

from _accept_cases import MALFORMED, host_loop, random_cases, reference_walk


def test_reference_walk_is_the_host_loop_on_hand_made_trees():
    cases = {
        # a chain whose every drafted token is its parent's arg-max
        "chain": ([-1, 0, 1, 2, 3], [9, 5, 6, 7, 8], [5, 6, 7, 8, 1], [0, 1, 2, 3, 4]),
        # the chain breaks at node 3
        "broken chain": ([-1, 0, 1, 2, 3], [9, 5, 6, 0, 8], [5, 6, 7, 8, 1], [0, 1, 2]),
        # two children of the root carry the arg-max: the lower index wins, and the walk goes on below IT
        "two matching siblings": ([-1, 0, 0, 2, 1], [9, 5, 5, 6, 6], [5, 6, 6, 0, 0], [0, 1, 4]),
        # node 2 carries the root's arg-max but hangs off node 1: not a child, not accepted
        "a match at a non-child": ([-1, 0, 1], [9, 4, 5], [5, 0, 0], [0]),
        # node 1 is rejected; its child 2 would match node 1's arg-max, but the walk never gets there
        "a match below a rejected node": ([-1, 0, 1, 0], [9, 4, 6, 5], [5, 6, 0, 0], [0, 3]),
        "a single node": ([-1], [3], [3], [0]),
    }
    for name, (par, tok, am, want) in cases.items():
        assert host_loop(par, tok, am) == want, name
        assert reference_walk(par, tok, am, len(par)) == want, name
    # the cap cuts the path, nothing else
    par, tok, am, want = cases["chain"]
    for cap in range(1, 6):
        assert reference_walk(par, tok, am, cap) == want[:cap]
    assert reference_walk([], [], [], 4) == []


def test_reference_walk_is_the_host_loop_on_random_trees():
    for par, tok, am in random_cases():
        assert reference_walk(par, tok, am, len(par)) == host_loop(par, tok, am)


def test_reference_walk_terminates_on_malformed_parents():
    for par in MALFORMED:
        n = len(par)
        path = reference_walk(par, [0] * n, [0] * n, 64)
        assert path[0] == 0 and all(a < b for a, b in zip(path, path[1:])) and path[-1] < n and len(path) <= n, par
    assert reference_walk(MALFORMED[0], [0] * 6, [0] * 6, 64) == [0]          # node 1 names node 2, node 2 names node 1: nobody names 0
    assert reference_walk(MALFORMED[3], [0] * 6, [0] * 6, 64) == [0, 1, 3]    # lowest child first: 0 -> 1 (not 2, 5) -> 3 (not 4)


def test_random_cases_are_not_trivial():
    """Seed 11, n = 24, vocabulary 3, 200 trees.  Measured on the CPU: 21 % of the paths have length 1 and 43 % length >= 3 (the
    longest: 8 nodes)."""
    lens = [len(reference_walk(p, t, a, 24)) for p, t, a in random_cases(seed=11, n=24, vocab=3, count=200)]
    ones, long_ = sum(x == 1 for x in lens) / 200, sum(x >= 3 for x in lens) / 200
    print(f"random accept cases: {100 * ones:.1f} % of length 1, {100 * long_:.1f} % of length >= 3, longest {max(lens)}")
    assert ones >= 0.15 and long_ >= 0.30


def test_python_wrappers_raise_before_the_library_is_touched(built_lib):
    from qserve_amd import append as A
    i64, i32 = torch.int64, torch.int32
    tok, am, par = torch.zeros(6, dtype=i64), torch.zeros(6, dtype=i64), torch.zeros(6, dtype=i32)      # CPU tensors: every call must
    cu = torch.tensor([0, 6], dtype=i32)                                                                  # fail in the checks
    with pytest.raises(RuntimeError, match="scalar type"):
        A.accept_greedy(tok.to(i32), am, par, cu)
    with pytest.raises(RuntimeError, match="scalar type"):
        A.accept_greedy(tok, am, par.to(i64), cu)
    with pytest.raises(RuntimeError, match="scalar type"):
        A.accept_greedy(tok, am, par, cu.to(i64))
    with pytest.raises(TypeError):
        A.accept_greedy(tok, [0] * 6, par, cu)
    with pytest.raises(RuntimeError, match="one entry per node"):
        A.accept_greedy(tok, am[:5], par, cu)
    with pytest.raises(RuntimeError, match="one entry per node"):
        A.accept_greedy(tok.view(2, 3), am.view(2, 3), par.view(2, 3), cu)
    with pytest.raises(RuntimeError, match=r"batch \+ 1"):
        A.accept_greedy(tok, am, par, cu.view(1, 2))
    for bad in (0, 65, -1):
        with pytest.raises(RuntimeError, match=f"max_accept={bad}"):
            A.accept_greedy(tok, am, par, cu, max_accept=bad)
    out = (torch.zeros((1, 4), dtype=i32), torch.zeros(1, dtype=i32), torch.zeros(1, dtype=i64), torch.zeros(1, dtype=i64))
    with pytest.raises(RuntimeError, match="out must be"):
        A.accept_greedy(tok, am, par, cu, max_accept=5, out=out)                       # accept_idx [1, 4] for max_accept 5
    with pytest.raises(RuntimeError, match="out must be"):
        A.accept_greedy(tok, am, par, cu, max_accept=4, out=out[:3])
    with pytest.raises(RuntimeError, match="scalar type"):
        A.accept_greedy(tok, am, par, cu, max_accept=4, out=(out[0], out[1], out[2].to(i32), out[3]))
    with pytest.raises(RuntimeError, match="CUDA"):
        A.accept_greedy(tok, am, par, cu, max_accept=4, out=out)                       # everything right but the device

    Hkv = 2
    lt, past = torch.zeros(3, dtype=i64), torch.zeros(1, dtype=i32)
    idx, lens = torch.zeros((1, 4), dtype=i32), torch.zeros(1, dtype=i32)
    with pytest.raises(RuntimeError, match="scalar type"):
        A.commit_path_layers(lt.to(i32), past, idx, lens, 2, Hkv, Hkv * 64, True)
    with pytest.raises(RuntimeError, match="scalar type"):
        A.commit_path_layers(lt, past, idx.to(i64), lens, 2, Hkv, Hkv * 64, True)
    with pytest.raises(RuntimeError, match="at least one layer"):
        A.commit_path_layers(lt[:0], past, idx, lens, 2, Hkv, Hkv * 64, True)
    with pytest.raises(RuntimeError, match="at least one layer"):
        A.commit_path_layers(lt.view(1, 3), past, idx, lens, 2, Hkv, Hkv * 64, True)
    with pytest.raises(RuntimeError, match="accept_idx"):
        A.commit_path_layers(lt, past, idx.view(4), lens, 2, Hkv, Hkv * 64, True)
    with pytest.raises(RuntimeError, match="accept_idx"):
        A.commit_path_layers(lt, past, idx, torch.zeros(2, dtype=i32), 2, Hkv, Hkv * 64, True)
    with pytest.raises(RuntimeError, match="max_accept=65"):
        A.commit_path_layers(lt, past, torch.zeros((1, 65), dtype=i32), lens, 2, Hkv, Hkv * 64, True)
    with pytest.raises(RuntimeError, match="max_blocks=0"):
        A.commit_path_layers(lt, past, idx, lens, 0, Hkv, Hkv * 64, True)
    with pytest.raises(RuntimeError, match="size_per_token"):
        A.commit_path_layers(lt, past, idx, lens, 2, Hkv, Hkv * 128, True)
    with pytest.raises(RuntimeError, match="CUDA"):
        A.commit_path_layers(lt, past, idx, lens, 2, Hkv, Hkv * 64, True)
    with pytest.raises(RuntimeError, match="at least one layer"):
        A.layer_table_pointers([])
    with pytest.raises(RuntimeError, match="one shape"):
        A.layer_table_pointers([torch.zeros((1, 2, 2), dtype=i64), torch.zeros((1, 2, 3), dtype=i64)])
    with pytest.raises(RuntimeError, match="CUDA"):
        A.layer_table_pointers([torch.zeros((1, 2, 2), dtype=i64)])


def test_accept_entry_validates_before_any_device_call(built_lib):
    from qserve_amd._lib import lib

    def call(tok=8, am=16, par=4, cu=4, T=6, B=1, ma=6, idx=4, lens=4, last=8, nxt=8):
        return lib.qs_tree_accept_greedy(tok, am, par, cu, T, B, ma, idx, lens, last, nxt, None)

    for null in ("tok", "am", "par", "cu", "idx", "lens"):
        assert call(**{null: 0}) == -1 and b"null" in lib.qs_last_error(), null
    assert call(T=-1) == -1 and call(B=-1) == -1 and b"bad sizes" in lib.qs_last_error()
    assert call(ma=0) == -1 and b"max_accept=0" in lib.qs_last_error()
    assert call(ma=65) == -1 and b"max_accept=65" in lib.qs_last_error()
    for odd in ("tok", "am", "last", "nxt"):
        assert call(**{odd: 12}) == -1 and b"8-byte" in lib.qs_last_error(), odd
    assert call(B=0) == 0 and call(T=0) == 0                              # nothing to do: no launch
    assert call(B=0, last=0, nxt=0) == 0                                  # the two optional outputs may be null


def test_commit_layers_entry_validates_before_any_device_call(built_lib):
    from qserve_amd._lib import lib

    def call(lt=8, L=3, past=4, idx=4, lens=4, B=1, ma=4, mb=2, Hkv=2, tpb=64, spt=2 * 64, int4=1, zeros=1):
        return lib.qs_kv_cache_commit_path_layers(lt, L, past, idx, lens, B, ma, mb, Hkv, tpb, spt, int4, zeros, None)

    for null in ("lt", "past", "idx", "lens"):
        assert call(**{null: 0}) == -1 and b"null" in lib.qs_last_error(), null
    assert call(lt=12) == -1 and b"8-byte" in lib.qs_last_error()
    assert call(L=0) == -1 and b"num_layers=0" in lib.qs_last_error() and call(L=-2) == -1
    assert call(ma=65) == -1 and b"64" in lib.qs_last_error()
    assert call(Hkv=0) == -1 and call(Hkv=3) == -1 and call(spt=2 * 128) == -1 and call(mb=0) == -1 and call(ma=-1) == -1 and call(B=-1) == -1
    assert call(tpb=32) == -2 and call(zeros=0) == -2
    assert call(B=0) == 0 and call(ma=0) == 0                             # nothing to do: no launch
