"""DecodeEngine with `sliding_window` on the GPU: a window that never binds, and a binding window under capture."""
import pytest
import torch

pytestmark = pytest.mark.gpu
STEPS, MARGIN = 4, 4.486        # test_a_window_that_never_binds has the measurement


def _engine(prompt, window, chunk=None):
    from qserve_amd import decode as D
    cfg = dict(D.TINY, sliding_window=window) if window else D.TINY
    eng = D.DecodeEngine(cfg, batch=2, prompt_len=prompt, max_new=8, device="cuda:0")
    eng.prefill(prompt) if chunk is None else eng.prefill_chunked(prompt, chunk)
    return eng


def _finals(eng, runs=None):
    out = [eng.final.float().clone()]
    for run in runs or [eng.step] * STEPS:
        run()
        out.append(eng.final.float().clone())
    torch.cuda.synchronize()
    return torch.stack(out)


def test_a_window_that_never_binds(gpu):
    """TINY, prompt 40, four steps, sliding_window = 64 (longer than the text) against the same engine without it: `final` after the
    prompt and after every step; the two differ in kernels and in where the quantiser runs, not in mathematics.  Margin: the largest
    |final difference| between two EXISTING paths of that kind, prefill against prefill_chunked(chunk = 16), each followed by the
    same four steps, measured on the parent commit's paths: 4.486 (2026-11-26, MI355X; after the prompt and each step: 0.242, 3.50,
    4.49, 3.89, 0.572 - from the first step on a greedy token of the two runs differs, and `final` with it); four times that is
    allowed, because the new pair differs from both in kernel and in quantiser placement.  The windowed engine measured 0.077
    against the plain one on the same day."""
    plain, win = _finals(_engine(40, 0)), _finals(_engine(40, 64))
    got = float((win - plain).abs().max())
    print(f"WINDOW engine: windowed vs plain max |final difference| {got:.4e} (allowed {4 * MARGIN:.4e})")
    assert torch.isfinite(win).all() and got <= 4 * MARGIN, f"windowed engine differs from the plain one by {got:.3e} (allowed {4 * MARGIN:.3e})"


def test_captured_step_under_a_binding_window(gpu):
    """Prompt 150 with sliding_window = 64: the captured step replays bit-equal to the eager steps."""
    eager, cap = _finals(_engine(150, 64)), _engine(150, 64)
    got = _finals(cap, [cap.capture] + [cap.run] * (STEPS - 1))      # (capture's warm-up is a real step)
    assert torch.equal(got, eager), "captured run differs from the eager steps"
