"""Where the RoPE cos / sin values come from (DESIGN.md "RoPE coefficient sources"): the library's per-device tables - 8 slots keyed by
(base, length), never freed - or the in-kernel evaluation, chosen per row by `table && pos < table_len`.  The design claims both give
the same bytes; the scenarios of tests/_rope_source_child.py pin that for the prefill, append and tree writers, both matrix-core decode
kernels and append attention, and read the source of every call from qs_debug_rope_table_state.  The table state is process-wide and
irreversible, so every scenario is a fresh child process under a time limit of its own, one at a time; nothing is re-executed."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("scenario", ["fresh", "short_table", "boundary_writers", "capture", "exhausted", "interleaved"])
def test_rope_sources_give_the_same_bytes(gpu, scenario):
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tests", "_rope_source_child.py"), scenario], cwd=ROOT,
                       capture_output=True, text=True)
    print("\n".join(l for l in r.stdout.splitlines() if l.startswith(("[rope-source]", "ROPE-SOURCE-OK"))))
    assert r.returncode == 0 and f"ROPE-SOURCE-OK {scenario}" in r.stdout, f"exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-4000:]}"
