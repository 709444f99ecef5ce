"""RoPE frequency profiles on the GPU (DESIGN.md "RoPE frequency profiles"): the key of a registered profile - llama3 with all three
bands populated, YaRN with mscale != 1 - goes wherever a rotary base goes, and every writer and decode kernel gives the bytes of the numpy
restatement (tests/_rope_scaling_cases.py), from a table, from the in-kernel evaluation and inside a capture; plain bases keep their
bytes and their table slots.  Profiles and tables are process-wide and never freed, so every scenario of tests/_rope_scaling_child.py is
a fresh child process under a time limit of its own, one at a time; nothing is re-executed."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("scenario", ["table", "beyond", "capture", "plain"])
def test_profile_key_in_place_of_the_base(gpu, scenario):
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tests", "_rope_scaling_child.py"), scenario], cwd=ROOT,
                       capture_output=True, text=True)
    print("\n".join(l for l in r.stdout.splitlines() if l.startswith(("[rope-scaling]", "ROPE-SCALING-OK"))))
    assert r.returncode == 0 and f"ROPE-SCALING-OK {scenario}" in r.stdout, f"exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-4000:]}"
