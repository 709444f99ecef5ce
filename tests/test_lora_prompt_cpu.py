"""The prompt LoRA rows on the CPU: the planner's form on both sides of each of its new limits (csrc/lora_plan.h through
`lora.rows_form`), the run-length function of the shrink grid (every K slice in exactly one run), and three refusals of
`qs_lora_rows_prompt`, which answers before any device call."""
import pytest

from test_lora_rows_cpu import OK

MIN_RPS, MIN_ROWS = 17, 4096                            # lora_plan.h: PROMPT_MIN_ROWS_PER_SEQ, PROMPT_MIN_ROWS


@pytest.fixture(scope="module")
def lora(built_lib):
    from qserve_amd import lora
    return lora


@pytest.mark.parametrize("T, rps, slots, form", [
    (MIN_ROWS, 32, 8, "prompt"), (MIN_ROWS - 32, 32, 8, "rows"),                        # T >= PROMPT_MIN_ROWS
    (MIN_RPS * 241, MIN_RPS, 8, "prompt"), (MIN_RPS * 240, MIN_RPS, 8, "rows"), ((MIN_RPS - 1) * 256, MIN_RPS - 1, 8, "rows"),   # rows_per_seq >= 17
    (16384, 1024, 100, "prompt"), (16384, 16384, 1, "prompt"),                          # no slot limit; one sequence
    (4096, 16, 8, "rows"), (15 * 512, 15, 8, "grouped")])                                # what the other forms keep
def test_rows_form_on_both_sides_of_each_prompt_limit(lora, T, rps, slots, form):
    assert lora.FORMS == ("rows", "grouped", "prompt") and lora.rows_form(T, rps, slots) == form


def test_a_planned_prompt_form_holds_up_to_rank_16(built_lib):
    from qserve_amd._lib import lib
    assert [lib.qs_lora_rows_form_for_rank(2, r) for r in (8, 16, 32, 64)] == [2, 2, 0, 0]
    assert all(lib.qs_lora_rows_form_for_rank(f, r) == f for f in (0, 1) for r in (8, 16, 32, 64)) and lib.qs_lora_rows_form_for_rank(3, 16) == -1


@pytest.mark.parametrize("tiles, kslices", [(1, 1), (1, 28), (16, 8), (64, 28), (200, 28), (256, 8), (1024, 8), (4096, 28), (3, 2048)])
def test_runs_cover_every_slice_exactly_once(built_lib, tiles, kslices):
    """The kernel's walk - workgroup y takes slices y * run .. min(y * run + run, K slices) - 1 of ceil(K slices / run) workgroups -
    against the list of slices; few tiles: short runs, many tiles: one run over all of K."""
    from qserve_amd._lib import lib
    run = lib.qs_lora_rows_prompt_run(tiles, kslices)
    assert 1 <= run <= kslices
    runs = -(-kslices // run)
    walked = [sl for y in range(runs) for sl in range(y * run, min(y * run + run, kslices))]
    assert walked == list(range(kslices)) and (runs - 1) * run < kslices
    assert run == (1 if tiles * kslices <= 1024 else kslices if tiles >= 1024 else run)


@pytest.mark.parametrize("kw, msg", [(dict(out=0), b"null pointer"), (dict(r=12), b"r=12"), (dict(T=45, rps=15), b"rows_per_seq < 16")])
def test_prompt_entry_refuses_before_any_device_call(built_lib, kw, msg):
    """QS_EINVAL with a message under the entry's own name; the addresses are never dereferenced.  T = 0 with good arguments is QS_OK."""
    from qserve_amd._lib import lib

    def call(**kw):
        a = {**OK, "T": 48, "rps": 16, **kw}
        return lib.qs_lora_rows_prompt(a["out"], a["ostride"], a["x"], a["xstride"], a["xs"], a["A"], a["B"], a["sc"], a["ids"], a["slots"],
                                       a["T"], a["K"], a["N"], a["r"], a["rps"], a["nseg"], a["e0"], a["e1"], a["e2"], a["ws"], a["wsb"], None)

    assert call(T=0) == 0
    assert call(**kw) == -1
    err = lib.qs_last_error()
    assert err.startswith(b"lora_rows_prompt:") and msg in err, err
