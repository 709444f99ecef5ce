"""Record tests/golden/lora_bits.json: for every case of the three LoRA GPU tests (every name of `_lora_cases.SHAPES` under
form="rows", of `CASES` of tests/test_lora_grouped_gpu.py under "grouped", of `CASES` of tests/test_lora_prompt_gpu.py under "prompt")
the SHA-256 of the case's inputs and of the whole out_store after `lora.lora_rows(..., form=)`, with the tests' own case builders.

The bits are those of the library named by QS_AMD_LIBRARY, which must be a build of the PARENT of the commit that changes the
kernels - never of the tree under test, or the pin pins nothing:

    QS_AMD_LIBRARY=<the parent's libqserve_amd.so> python scripts/record_lora_bits.py [--out tests/golden/lora_bits.json]

The committed file was recorded on an MI355X against a build of commit 69ffe3b ("Test the grouped MoE tile on wide grids, deep K and
extreme operands"), the last one with the rows form and the grouped form in translation units of their own.  Re-record only when a
test reports "inputs drifted" (the case builders or numpy's generators changed), and then again at that commit's kernels."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "lora_bits.json"))
    a = ap.parse_args()
    assert os.environ.get("QS_AMD_LIBRARY"), "name the parent commit's library through QS_AMD_LIBRARY"
    import torch
    assert torch.cuda.is_available(), "record_lora_bits needs a GPU"
    import _lora_cases as K
    import test_lora_grouped_gpu as G
    import test_lora_prompt_gpu as P
    from qserve_amd import _lib, lora
    gpu = torch.device("cuda:0")
    forms = {"rows": [(n, K.make_case(n)) for n in sorted(K.SHAPES)],
             "grouped": [(n, G._case(n)) for n in sorted(G.CASES)],
             "prompt": [(n, P._case(n)) for n in sorted(P.CASES)]}
    rec = {}
    for form, cases in forms.items():
        rec[form] = {}
        for name, c in cases:
            out, out_store, _, rest = G._device(c, gpu)
            lora.lora_rows(out, *rest, form=form)
            torch.cuda.synchronize()
            rec[form][name] = {"inputs": K.input_digest(c), "out_store": K.store_digest(out_store.cpu().numpy())}
            print(f"{form:8s} {name:40s} {rec[form][name]['out_store'][:16]}", flush=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {sum(len(v) for v in rec.values())} cases with {_lib.LIB_PATH} -> {a.out}")


if __name__ == "__main__":
    main()
