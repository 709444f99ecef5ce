"""GPU tests of the constrained-decoding kernels (qserve_amd.constraints, csrc/constrain_rows.hip) on the cases of
tests/_constraint_cases.py: bit-equality with the numpy restatement over the WHOLE stored buffer - the padding's canaries and the rows
of unconstrained states included -, and two runs bit-identical.  What each case plants:

    min_vocab           n_vocab = 8, S = 2, C = 1; row states -1, -2 and S (out of range: untouched), an all-allowed and a none-allowed state
    odd_tail            n_vocab = 12 at stride 16: the last n_vocab % 8 ids go one by one, the padding behind them is neither read nor written
    two_vectors_c3      n_vocab = 33 000 at stride 33 008, C = 3 with next_stride 5: nine slices of one pass, the last partial; classes -1, C,
                        32 767 and -32 768; negative entries other than -1; logits with -inf, +-0, positive and negative values
    two_vectors_c32768  the same at C = 32 768 (the largest: the whole 4 KiB mask is staged) with next_stride 32 776, four rows: nine
                        slices of one pass again, the rows being few; classes 0, 31, 32 and 32 767
    big_vocab           n_vocab = 128 256 once: B = 2, n = 4 -> 8 rows, C = 256: 32 slices of one pass
    passes_2            SEVERAL PASSES per workgroup, what a verification at C > 1024 launches: n_vocab = 33 003 (n_vocab % 8 = 3) at stride
                        33 008, 128 rows at C = 32 768 -> slices of 8192 ids, two passes; the fifth slice holds 235 ids, 3 of them the tail
    passes_5            the same vocabulary, 512 rows at C = 8192 with next_stride 8200 -> slices of 20 480 ids, five passes (the loop is
                        unrolled by two); the second slice holds three full passes, a partial one and the tail; classes in contiguous
                        runs of ids, out-of-range classes at the seams of passes and slices
                        (tests/_constraint_cases.py SLICES pins what each case launches; tests/test_constrain_rows_cpu.py checks it)
    node_states         the 12-node tree of tests/_accept_engine.py (siblings with different tokens; tokens -1, n_vocab and 2^40; classes
                        -1 and C; a disallowed node whose children are all dead; unconstrained roots -1 and S), a 64-node chain that lives
                        to its end, malformed parents, a tree of the root alone
    advance             k = 0 (not written), k = m, clipped 1 <= k < m, k beyond max_accept and negative, accept_idx out of range (clamped),
                        next_token out of the vocabulary (dead), unconstrained and dead path states, accept_lens null, a plain step"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROW_CASES = ("min_vocab", "odd_tail", "two_vectors_c3", "two_vectors_c32768", "big_vocab", "passes_2", "passes_5")
NODE_CASES = ("par12", "chain64", "malformed", "root_only")
ADVANCE_CASES = ("path", "path_no_lens", "step", "step_k")


def _dev(a, gpu):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _tables(case, gpu):
    """The tables on the device, `next` as the padded store's first C columns."""
    return _dev(case["token_class"], gpu), _dev(case["next"], gpu)[:, :case["C"]]


@pytest.fixture(scope="module")
def row_cases():
    """name -> (case, the restatement's bits): computed once, never changed."""
    from _constraint_cases import restate_rows, row_cases
    return {k: (c, restate_rows(c["store"], c["n_vocab"], c["row_state"], c["token_class"], c["next"], c["C"])) for k, c in row_cases().items()}


def _run_rows(case, gpu):
    from qserve_amd.constraints import constrain_rows
    store = _dev(case["store"].view(np.int16), gpu).view(torch.float16)
    tc, nx = _tables(case, gpu)
    out = constrain_rows(store[:, :case["n_vocab"]], _dev(case["row_state"], gpu), tc, nx)
    assert out.data_ptr() == store.data_ptr()
    torch.cuda.synchronize()
    return store.view(torch.int16).cpu().numpy().view(np.uint16)


def test_the_cases_are_the_documented_ones(row_cases):
    from _constraint_cases import advance_cases, node_cases
    assert tuple(row_cases) == ROW_CASES and tuple(node_cases()) == NODE_CASES and tuple(advance_cases()) == ADVANCE_CASES


@pytest.mark.parametrize("name", ROW_CASES)
def test_rows_against_the_restatement(gpu, row_cases, name):
    case, want = row_cases[name]
    got = _run_rows(case, gpu)
    diff = np.argwhere(got != want)
    masked = int((want != case["store"]).sum())
    print(f"{name}: {len(diff)} of {got.size} elements differ from the restatement; the rule masks {masked}")
    assert len(diff) == 0, f"{name}: first difference at (row, id) {diff[0].tolist()}: {got[tuple(diff[0])]:#06x} != {want[tuple(diff[0])]:#06x}"
    assert masked > 0 and (want[:, case["n_vocab"]:] == 0x7BFF).all()
    assert np.array_equal(_run_rows(case, gpu), got), f"{name}: two runs differ"


@pytest.mark.parametrize("name", NODE_CASES)
def test_node_states_against_the_restatement(gpu, name):
    from _constraint_cases import node_cases, restate_node_states
    from qserve_amd.constraints import node_states
    c = node_cases()[name]
    want = restate_node_states(c["state"], c["node_tokens"], c["parents"], c["token_class"], c["next"], c["C"])
    tc, nx = _tables(c, gpu)
    B, n = c["node_tokens"].shape
    out = torch.full((B + 1, n), 77, dtype=torch.int32, device=gpu)          # (a canary row behind the output)
    args = (_dev(c["state"], gpu), _dev(c["node_tokens"], gpu), torch.tensor(c["parents"], dtype=torch.int32, device=gpu), tc, nx)
    got = node_states(*args, out=out[:B])
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and np.array_equal(out[:B].cpu().numpy(), want), f"{name}: node states differ"
    assert bool((out[B] == 77).all())
    assert torch.equal(node_states(*args), out[:B]), f"{name}: two runs differ"


@pytest.mark.parametrize("name", ADVANCE_CASES)
def test_advance_against_the_restatement(gpu, name):
    from _constraint_cases import advance_cases, restate_advance
    from qserve_amd.constraints import advance
    c = advance_cases()[name]
    want = restate_advance(c["state"], c["node_state"], c["accept_idx"], c["accept_lens"], c["next_token"], c["token_class"], c["next"],
                           c["C"], c["max_accept"])
    tc, nx = _tables(c, gpu)
    for _ in range(2):                                                        # two runs from the same input
        state = _dev(c["state"], gpu)
        got = advance(state, _dev(c["next_token"], gpu), tc, nx, node_state=_dev(c["node_state"], gpu), accept_idx=_dev(c["accept_idx"], gpu),
                      accept_lens=_dev(c["accept_lens"], gpu))
        torch.cuda.synchronize()
        assert got.data_ptr() == state.data_ptr() and np.array_equal(state.cpu().numpy(), want), f"{name}: states differ"
    assert (want != c["state"]).any() and (want == c["state"]).any()


def test_einval_through_the_wrappers_writes_nothing(gpu):
    """What the wrappers' own checks let through and the library refuses: QS_EINVAL before any device call, surfaced with the library's
    message; nothing is launched, nothing written."""
    from qserve_amd.constraints import advance, constrain_rows, node_states
    tc = torch.zeros(24, dtype=torch.int16, device=gpu)
    nx = torch.full((2, 3), -1, dtype=torch.int32, device=gpu)
    rs = torch.zeros(2, dtype=torch.int32, device=gpu)
    logits = torch.ones((2, 24), dtype=torch.float16, device=gpu)
    with pytest.raises(RuntimeError, match=r"token_class must be 16-byte.*\(code -1\)"):
        constrain_rows(logits[:, :16], rs, tc[4:20], nx)                      # a misaligned class table
    buf = torch.ones((2 * 24 + 8,), dtype=torch.float16, device=gpu)
    with pytest.raises(RuntimeError, match=r"logits must be 16-byte.*\(code -1\)"):
        constrain_rows(buf[4:4 + 48].view(2, 24), rs, tc, nx)                 # misaligned rows
    with pytest.raises(RuntimeError, match=r"token_class must be 16-byte.*\(code -1\)"):
        node_states(rs, torch.zeros((2, 3), dtype=torch.int64, device=gpu), torch.zeros(3, dtype=torch.int32, device=gpu), tc[4:20], nx)
    with pytest.raises(RuntimeError, match=r"token_class must be 16-byte.*\(code -1\)"):
        advance(rs, torch.zeros(2, dtype=torch.int64, device=gpu), tc[4:20], nx)
    torch.cuda.synchronize()
    assert bool((logits == 1).all()) and bool((buf == 1).all()) and bool((rs == 0).all())
    constrain_rows(logits, rs, tc, nx)                                        # the same call, aligned: state 0 allows nothing
    assert bool(torch.isneginf(logits).all())
