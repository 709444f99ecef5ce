"""The grouped LoRA rows on the CPU: the planner's form on both sides of each of its limits (csrc/lora_plan.h through `lora.rows_form`),
the grid's tile bound against a brute-force count over every id assignment of small batches, and three refusals of
`qs_lora_rows_grouped`, which answers before any device call."""
import itertools

import pytest

from test_lora_rows_cpu import OK

MAX_SEQS = 16384                                        # lora_plan.h: GROUPED_MAX_SEQS


@pytest.fixture(scope="module")
def lora(built_lib):
    from qserve_amd import lora
    return lora


@pytest.mark.parametrize("T, rps, slots, form", [
    (256, 1, 8, "grouped"), (255, 1, 8, "rows"), (64, 1, 8, "rows"), (768, 12, 8, "rows"), (0, 1, 8, "rows"),   # S >= 256 (lora_plan.h: why)
    (15 * 256, 15, 8, "grouped"), (16 * 256, 16, 8, "rows"),                                # rows_per_seq < 16
    (256, 1, 64, "grouped"), (256, 1, 65, "rows"),                                          # slots <= 64
    (MAX_SEQS, 1, 8, "grouped"), (MAX_SEQS + 1, 1, 8, "rows"), (2 * MAX_SEQS, 2, 8, "grouped"), (2 * MAX_SEQS + 2, 2, 8, "rows")])
def test_rows_form_on_both_sides_of_each_limit(lora, T, rps, slots, form):
    assert lora.rows_form(T, rps, slots) == form


def test_rows_form_refuses_sizes_that_are_none(lora):
    for args in ((-1, 1, 8), (64, 0, 8), (64, 3, 8), (64, 1, 0)):
        with pytest.raises(RuntimeError, match="lora_rows_form"):
            lora.rows_form(*args)
    with pytest.raises(RuntimeError, match="form='tiles'"):
        lora.lora_rows(*[None] * 9, form="tiles")


def test_the_tile_bound_holds_for_every_assignment_and_is_reached(built_lib):
    """ceil(T / 16) + min(slots, S) - 1 against sum_a ceil(rows of a / 16) over every assignment of -1 .. slots-1 to S <= 6 sequences,
    slots <= 3, at rows_per_seq 1, 5 and 15: never exceeded, and reached by some assignment whenever the rows can be split that way."""
    from qserve_amd._lib import lib
    for S, slots, rps in itertools.product(range(1, 7), range(1, 4), (1, 5, 15)):
        bound = lib.qs_lora_rows_grouped_tiles(S * rps, rps, slots)
        assert bound == -(-S * rps // 16) + min(slots, S) - 1
        worst = max(sum(-(-ids.count(a) * rps // 16) for a in range(slots)) for ids in itertools.product(range(-1, slots), repeat=S))
        assert worst <= bound, (S, slots, rps, worst, bound)
        if rps == 1 or slots == 1:                       # (single rows beside one big group: the assignment of the bound's proof)
            assert worst == bound, (S, slots, rps, worst, bound)
    assert lib.qs_lora_rows_grouped_tiles(20, 1, 4) == 5 and lib.qs_lora_rows_grouped_tiles(0, 1, 4) == 0


@pytest.mark.parametrize("kw, msg", [(dict(out=0), b"null pointer"), (dict(r=12), b"r=12"), (dict(slots=65), b"slots outside 1 .. 64")])
def test_grouped_entry_refuses_before_any_device_call(built_lib, kw, msg):
    """QS_EINVAL with a message under the entry's own name; the addresses are never dereferenced.  T = 0 with good arguments is QS_OK."""
    from qserve_amd._lib import lib

    def call(**kw):
        a = {**OK, **kw}
        return lib.qs_lora_rows_grouped(a["out"], a["ostride"], a["x"], a["xstride"], a["xs"], a["A"], a["B"], a["sc"], a["ids"], a["slots"],
                                        a["T"], a["K"], a["N"], a["r"], a["rps"], a["nseg"], a["e0"], a["e1"], a["e2"], a["ws"], a["wsb"], None)

    assert call(T=0) == 0
    assert call(**kw) == -1
    err = lib.qs_last_error()
    assert err.startswith(b"lora_rows_grouped:") and msg in err, err
