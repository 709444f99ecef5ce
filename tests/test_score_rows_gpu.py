"""qs_score_rows on the GPU against float64 log_softmax / argmax of hidden.double() @ lm_head.double().T on the CPU, at the smallest shapes
where the walk can go wrong: rows and V on both sides of a tile (TR = 128, TV = 256), K at one stage, at the ring's depth D = 3 and one
beyond, padded row strides, a vocabulary of six tiles plus one column cut into three splits, targets on the edges of tiles and splits,
-1 and V, a lone far maximum in the last and in the first split, bit-equal duplicated lm_head rows in different tiles and splits,
repeatability and one capture.

Tolerance (DESIGN.md "Scoring prompts"), per row from the float64 side: a logit is off by at most e = 2 (K + 4) 2^-24 max_i sum_k
|h_k w_ik| (fp16 products are exact in fp32, one rounding per accumulation step; the constant is the LoRA tests'), lp = x_t - lse
carries that twice, and the softmax stage adds qs_logprob_rows' 1e-5 + 2^-21 |lp|."""
import pytest
import torch

pytestmark = pytest.mark.gpu
TR, TV, D = 128, 256, 3
# name -> (rows, V, K, hidden row padding, lm_head row padding, forced splits)
CASES = {
    "one_row_v8": (1, 8, 64, 0, 0, 0),
    "under_a_tile": (TR - 1, TV - 1, 64 * D, 0, 0, 0),
    "over_a_tile_padded": (TR + 1, TV + 1, 64 * (D + 1), 8, 24, 0),
    "three_splits": (TR + 1, 6 * TV + 1, 64, 0, 0, 0),                    # 7 tiles: the planner's own cut is 3 + 3 + 1
    "seven_forced_splits": (5, 6 * TV + 1, 128, 16, 0, 7),
}
DUPES = (40, TV + 44, 3 * TV + 132)                                       # tile 0 / tile 1 (split 0), tile 3 (split 1); three different waves


def make(name):
    """-> hidden, lm_head (fp16 CPU views with the case's row strides), targets int32, and the float64 reference."""
    rows, V, K, hpad, wpad, _ = CASES[name]
    g = torch.Generator().manual_seed(sorted(CASES).index(name))
    hidden = torch.zeros((rows, K + hpad), dtype=torch.float16)[:, :K]
    lm_head = torch.zeros((V, K + wpad), dtype=torch.float16)[:, :K]
    hidden.copy_(torch.randn((rows, K), generator=g))
    lm_head.copy_(torch.randn((V, K), generator=g) * 0.1)
    targets = torch.randint(0, V, (rows,), generator=g).to(torch.int32)
    if V > 3 * TV + 132 and rows >= 5:
        # rows 0 .. 2 each own eight k where every other row is 0, so a planted column stands out (+ 32) in its row alone
        hidden[:, :24] = 0
        hidden[0, 0:8] = hidden[1, 8:16] = hidden[2, 16:24] = 4
        lm_head[V - 1, 0:8] = 1                                           # row 0: a lone maximum in the last split rescales every earlier partial
        lm_head[5, 8:16] = 1                                              # row 1: in the first split
        lm_head[DUPES[0], 16:24] = 1                                      # row 2: its maximum is a three-way tie
        lm_head[DUPES[1]] = lm_head[DUPES[2]] = lm_head[DUPES[0]]
        edges = [0, TV - 1, TV, 3 * TV - 1, 3 * TV, V - 1, V - 2]         # first / last column of a tile, of a split, of the vocabulary
        targets[:5] = torch.tensor([V - 1, -1, DUPES[1], V, DUPES[2]], dtype=torch.int32)
        targets[5:5 + min(rows - 5, len(edges))] = torch.tensor(edges[:rows - 5], dtype=torch.int32)
    x = hidden.double() @ lm_head.double().T
    absx = hidden.double().abs() @ lm_head.double().abs().T
    return hidden, lm_head, targets, dict(x=x, logp=torch.log_softmax(x, dim=1), lse=torch.logsumexp(x, dim=1),
                                          e=2.0 * (K + 4) * 2.0 ** -24 * absx.max(dim=1).values)


@pytest.fixture(scope="module")
def problems(gpu):
    out = {}
    for name in CASES:
        hidden, lm_head, targets, ref = make(name)
        dev = lambda t: torch.empty_strided(t.shape, t.stride(), dtype=t.dtype, device=gpu).copy_(t)   # noqa: E731  (keeps the padding)
        out[name] = (dev(hidden), dev(lm_head), targets.to(gpu), targets, ref)
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_score_rows_against_float64(problems, name):
    from qserve_amd.logprobs import score_plan, score_rows
    hidden, lm_head, tgt_d, targets, ref = problems[name]
    rows, V, K, _, _, splits = CASES[name]
    plan = score_plan(rows, V, K, splits)
    assert (plan["tile_rows"], plan["tile_vocab"], plan["depth"]) == (TR, TV, D)
    assert plan["splits"] == {"three_splits": 3, "seven_forced_splits": 7}.get(name, 1)
    lp, greedy, lse = (t.cpu() for t in score_rows(hidden, lm_head, tgt_d, lse=True, _splits=splits))
    scored = (targets >= 0) & (targets < V)
    assert torch.isnan(lp[~scored]).all() and torch.isfinite(lp[scored]).all()
    want = ref["logp"][scored, targets[scored].long()]
    bound = 2 * ref["e"][scored] + 1e-5 + 2.0 ** -21 * want.abs()
    err = (lp[scored].double() - want).abs()
    lse_err = (lse.double() - ref["lse"]).abs() / (ref["e"] + 1e-5 + 2.0 ** -21 * ref["lse"].abs())
    print(f"{name}: max |lp - exact| / bound = {(err / bound).max():.4f}, lse {lse_err.max():.4f}")
    assert (err <= bound).all() and (lse_err <= 1).all()
    # greedy: the float64 arg-max where its margin is clear, else an index whose exact logit is within that distance of the maximum
    top2 = ref["x"].topk(2, dim=1).values
    row_bound = 2 * (2 * ref["e"] + 1e-5)
    clear = top2[:, 0] - top2[:, 1] > row_bound
    assert clear.sum() >= 0.9 * rows - 1                                   # (- 1: the row whose maximum is a tie by construction)
    assert (greedy[clear].long() == ref["x"].argmax(dim=1)[clear]).all()
    assert ((greedy >= 0) & (greedy < V)).all()
    assert (top2[:, 0] - ref["x"][torch.arange(rows), greedy.long()] <= row_bound).all()


def test_duplicated_rows_tie_bit_for_bit_and_runs_repeat(problems):
    """Bit-equal lm_head rows in different tiles and splits: greedy names the lowest index, the duplicates' lp are bit-equal; and two runs
    on the same inputs give the same bits."""
    from qserve_amd.logprobs import score_rows
    hidden, lm_head, tgt_d, _, _ = problems["three_splits"]
    runs = [score_rows(hidden, lm_head, torch.full_like(tgt_d, d), lse=True) for d in DUPES + (DUPES[0],)]
    assert int(runs[0][1][2]) == DUPES[0]
    for lp, greedy, lse in runs[1:]:
        assert torch.equal(lp, runs[0][0]) and torch.equal(greedy, runs[0][1]) and torch.equal(lse, runs[0][2])


def test_capture_replays_the_eager_bits(problems):
    from qserve_amd.logprobs import score_rows
    hidden, lm_head, tgt_d, _, _ = problems["three_splits"]
    eager = score_rows(hidden, lm_head, tgt_d, lse=True)                 # (also: the workspace exists before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = score_rows(hidden, lm_head, tgt_d, lse=True)
    for _ in range(3):
        for t in captured:
            t.fill_(0)
        graph.replay()
        torch.cuda.synchronize()
        # (lp holds NaN where a target is out of range: compare bits)
        assert all(torch.equal(c.view(torch.int32), e.view(torch.int32)) for c, e in zip(captured, eager))
