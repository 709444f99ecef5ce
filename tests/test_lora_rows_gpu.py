"""`lora.lora_rows` on the GPU against the float64 oracle of tests/_lora_cases.py under the derived tolerance
    |got - y| <= 2^-11 |y| + 2^-24 + 2 (K + r + 4) 2^-24 M,   M = scaling sum_j |B| x_scale sum_k |A| |x|
on every case of _lora_cases.SHAPES: T in {1, 3, 64, 130} (and 36, for rows_per_seq = 12, which divides none of those), rows_per_seq
in {1, 3, 5, 12, 65}, K in {128, 256, 4096, 14336}, N = 64 / 1024 in three segments / 28672 in two, every r, slots 1 and 4, adapters mixed
with -1, `slots` and -7.  x and out are views into sentinel-filled stores (a guard row on either side, padding behind every row) that must
come back untouched; rows of an adapter out of range must keep their bits.  Two runs and a graph replay must agree bit for bit; a zeroed
slot must leave the values as they are."""
import numpy as np
import pytest
import torch

import _lora_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lora(built_lib):
    from qserve_amd import lora
    return lora


def _device(c, gpu):
    """-> (the out view, its store, the argument tuple behind `out`) on the device."""
    T, Kk, N = c["T"], c["K"], c["N"]
    out_store, x_store = torch.from_numpy(c["out_store"]).to(gpu), torch.from_numpy(c["x_store"]).to(gpu)
    rest = (x_store[1:T + 1, :Kk], torch.from_numpy(c["x_scale"]).to(gpu), torch.from_numpy(c["A"]).to(gpu), torch.from_numpy(c["B"]).to(gpu),
            torch.from_numpy(c["scaling"]).to(gpu), torch.from_numpy(c["seq_adapter"]).to(gpu), c["rows_per_seq"], c["seg_ends"])
    return out_store[1:T + 1, :N], out_store, x_store, rest


@pytest.mark.parametrize("name", sorted(K.SHAPES))
def test_rows_against_the_oracle(gpu, lora, name):
    c = K.make_case(name)
    T, N = c["T"], c["N"]
    y, M, active = K.case_oracle(c)
    out, out_store, x_store, rest = _device(c, gpu)
    assert lora.lora_rows(out, *rest) is out
    torch.cuda.synchronize()
    got_store = out_store.cpu().numpy()
    got = got_store[1:T + 1, :N].astype(np.float64)
    err, tol = np.abs(got - y), K.tolerance(y, M, c["K"], c["r"])
    worst = np.unravel_index(np.argmax(err / tol), err.shape)
    print(f"{name}: max |got - y| / tolerance = {(err / tol).max():.4f} at {worst}; {int(active.sum())} of {T} rows under an adapter")
    assert np.isfinite(got).all() and (err <= tol).all(), f"{int((err > tol).sum())} values beyond the tolerance, the worst at {worst}"
    before = c["out_store"].view(np.uint16)
    after = got_store.view(np.uint16)
    assert np.array_equal(after[1:T + 1, :N][~active], before[1:T + 1, :N][~active]), "a row of an adapter out of range changed"
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[T + 1], before[T + 1]), "a guard row of out changed"
    assert np.array_equal(after[:, N:], before[:, N:]), "the padding behind out's rows changed"
    assert np.array_equal(x_store.cpu().numpy(), c["x_store"]), "x changed"
    if active.any():
        changed = (after[1:T + 1, :N][active] != before[1:T + 1, :N][active]).mean()
        assert changed > 0.5, "the adapters hardly changed their rows"


@pytest.mark.parametrize("name", ["step_64", "two_long_seqs", "mlp_wide"])
def test_two_runs_and_a_graph_replay_are_bit_identical(gpu, lora, name):
    """The same call twice on fresh copies of `out`, with a caller-provided workspace filled with different bytes in between, then
    captured in a hipGraph and replayed on a third copy: the same bits."""
    c = K.make_case(name)
    T, N = c["T"], c["N"]
    out, out_store, _, rest = _device(c, gpu)
    start = out_store.clone()
    ws = torch.empty((lora.workspace_bytes(T, c["K"], c["r"], len(c["seg_ends"])),), dtype=torch.uint8, device=gpu)
    ws.fill_(0x7F)
    lora.lora_rows(out, *rest, workspace=ws)
    first = out_store.clone()
    out_store.copy_(start)
    ws.fill_(0xFF)
    lora.lora_rows(out, *rest, workspace=ws)
    assert torch.equal(out_store.view(torch.int16), first.view(torch.int16)), "two runs differ"
    assert not torch.equal(first.view(torch.int16), start.view(torch.int16))
    out_store.copy_(start)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        lora.lora_rows(out, *rest, workspace=ws)
    out_store.copy_(start)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out_store.view(torch.int16), first.view(torch.int16)), "the graph replay differs from the eager run"


def test_a_zeroed_slot_leaves_the_values_unchanged(gpu, lora):
    """Slot 1 of the 64-row case zeroed the way LoraTable.unload zeroes it (A, B and scaling): its rows keep their values (a -0.0 may
    come back as +0.0), the rows of the other slots still change."""
    c = K.make_case("step_64")
    c["A"][1], c["B"][1], c["scaling"][1] = 0, 0, 0
    T, N = c["T"], c["N"]
    out, out_store, _, rest = _device(c, gpu)
    lora.lora_rows(out, *rest)
    got = out_store.cpu().numpy()[1:T + 1, :N]
    rows = np.repeat(c["seq_adapter"], c["rows_per_seq"])
    assert (rows == 1).sum() >= 4 and (rows == 0).sum() >= 4
    assert np.array_equal(got[rows == 1], c["out_store"][1:T + 1, :N][rows == 1])
    assert (got[rows == 0] != c["out_store"][1:T + 1, :N][rows == 0]).mean() > 0.5
