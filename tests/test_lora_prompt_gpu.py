"""`lora.lora_rows(..., form="prompt")` on the GPU: tiles of up to 64 rows of one sequence (csrc/lora_prompt.hip).  Every case against
the float64 oracle of tests/_lora_cases.py under its derived tolerance
    |got - y| <= 2^-11 |y| + 2^-24 + 2 (K + r + 4) 2^-24 M,   M = scaling sum_j |B| x_scale sum_k |A| |x|
and bit for bit against form="rows" on a fresh copy and against the bits recorded in tests/golden/lora_bits.json; x and out are views
into sentinel-filled stores (a guard row on either side, padding behind every row) that must come back untouched, rows of an id out
of range must keep their bits.  The cases are the smallest
shapes at which the form can go wrong; what each probes stands beside it.  A captured call must follow ids changed in place."""
import numpy as np
import pytest
import torch

import _lora_cases as K

pytestmark = pytest.mark.gpu

# name -> (T, rows_per_seq, K, N, seg_ends, r, slots, ids)
CASES = {
    "one_wave_block_one_chunk": (16, 16, 128, 64, (64,), 8, 1, [0]),                       # R = 8: a partly empty rank tile
    "full_tile_plus_one_row_tile": (130, 65, 256, 1024, (512, 768, 1024), 32, 4, [3, 1]),    # K = 256: a partial slice of two chunks
    "tiles_of_64_and_36_rows": (400, 100, 640, 1024, (512, 768, 1024), 16, 4, [-1, 2, 4, 0]),   # a block of 4 rows; one slice + one chunk
    "three_rank_groups": (128, 64, 256, 1024, (512, 768, 1024), 64, 1, [0, 0]),             # R = 192: the LDS staging at its bound
    "rank_rows_24": (48, 24, 128, 576, (64, 320, 576), 8, 2, [1, 0]),                       # N = 576: a short column slice, unequal segments
    "28_slices_56_column_slices": (32, 32, 14336, 28672, (14336, 28672), 16, 4, [2]),       # slices in slice order and in runs
    "nothing_changes": (64, 64, 128, 64, (64,), 8, 4, [-1]),
}


@pytest.fixture(scope="module")
def lora(built_lib):
    from qserve_amd import lora
    return lora


def _case(name):
    """The tensors of a case as `_lora_cases.make_case` lays them out: sentinel-filled stores, the tensors proper inside them."""
    T, rps, Kk, N, ends, r, slots, ids = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name))
    out_store = np.full((T + 2, N + 8), K.SENTINEL_H, dtype=np.float16)
    x_store = np.full((T + 2, Kk + 16), K.SENTINEL_X, dtype=np.int8)
    out_store[1:T + 1, :N] = rng.normal(0.0, 1.0, size=(T, N)).astype(np.float16)
    x_store[1:T + 1, :Kk] = rng.integers(-128, 128, size=(T, Kk), dtype=np.int8)
    return dict(T=T, rows_per_seq=rps, K=Kk, N=N, seg_ends=tuple(ends), r=r, slots=slots, seq_adapter=np.asarray(ids, dtype=np.int32),
                out_store=out_store, x_store=x_store, x_scale=rng.uniform(0.005, 0.05, size=T).astype(np.float16),
                A=rng.normal(0.0, 0.05, size=(slots, len(ends) * r, Kk)).astype(np.float16),
                B=rng.normal(0.0, 0.2, size=(slots, N, r)).astype(np.float16), scaling=rng.uniform(0.5, 2.0, size=slots).astype(np.float32))


def _device(c, gpu):
    T, Kk, N = c["T"], c["K"], c["N"]
    out_store, x_store = torch.from_numpy(c["out_store"]).to(gpu), torch.from_numpy(c["x_store"]).to(gpu)
    rest = [x_store[1:T + 1, :Kk]] + [torch.from_numpy(c[k]).to(gpu) for k in ("x_scale", "A", "B", "scaling", "seq_adapter")] + \
        [c["rows_per_seq"], c["seg_ends"]]
    return out_store[1:T + 1, :N], out_store, x_store, rest


@pytest.mark.parametrize("name", sorted(CASES))
def test_prompt_against_the_oracle_and_the_rows_form(gpu, lora, name):
    c = _case(name)
    T, N = c["T"], c["N"]
    y, M, active = K.case_oracle(c)
    out, out_store, x_store, rest = _device(c, gpu)
    rows_store = out_store.clone()
    assert lora.lora_rows(out, *rest, form="prompt") is out
    lora.lora_rows(rows_store[1:T + 1, :N], *rest, form="rows")
    torch.cuda.synchronize()
    got_store = out_store.cpu().numpy()
    got = got_store[1:T + 1, :N].astype(np.float64)
    err, tol = np.abs(got - y), K.tolerance(y, M, c["K"], c["r"])
    print(f"{name}: max |got - y| / tolerance = {(err / tol).max():.4f}; {int(active.sum())} of {T} rows under an adapter")
    assert np.isfinite(got).all() and (err <= tol).all(), f"{int((err > tol).sum())} values beyond the tolerance"
    assert torch.equal(out_store.view(torch.int16), rows_store.view(torch.int16)), "the prompt form differs from the rows form"
    before, after = c["out_store"].view(np.uint16), got_store.view(np.uint16)
    assert np.array_equal(after[1:T + 1, :N][~active], before[1:T + 1, :N][~active]), "a row of an adapter out of range changed"
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[T + 1], before[T + 1]), "a guard row of out changed"
    assert np.array_equal(after[:, N:], before[:, N:]), "the padding behind out's rows changed"
    assert np.array_equal(x_store.cpu().numpy(), c["x_store"]), "x changed"
    assert not active.any() or (after[1:T + 1, :N][active] != before[1:T + 1, :N][active]).mean() > 0.5, "the adapters hardly changed their rows"
    K.assert_recorded_bits("prompt", name, c, got_store)


def test_a_captured_call_follows_ids_changed_in_place(gpu, lora):
    """One prompt call captured in a hipGraph; seq_adapter rewritten in place (another adapter, and the base model where an adapter
    was); replays on fresh copies of `out` against an eager call under the new ids: the same bits, three times."""
    c = _case("full_tile_plus_one_row_tile")
    out, out_store, _, rest = _device(c, gpu)
    start, ids = out_store.clone(), rest[5]
    ws = torch.empty((lora.workspace_bytes(c["T"], c["K"], c["r"], len(c["seg_ends"])),), dtype=torch.uint8, device=gpu)
    lora.lora_rows(out, *rest, workspace=ws, form="prompt")
    old = out_store.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        lora.lora_rows(out, *rest, workspace=ws, form="prompt")
    ids.copy_(torch.tensor([-1, 2], dtype=torch.int32))
    out_store.copy_(start)
    lora.lora_rows(out, *rest, workspace=ws, form="prompt")
    want = out_store.clone()
    assert not torch.equal(want.view(torch.int16), old.view(torch.int16))
    for i in range(3):
        out_store.copy_(start)
        ws.fill_(0x7F + i)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out_store.view(torch.int16), want.view(torch.int16)), f"replay {i} differs from the eager call under the new ids"
