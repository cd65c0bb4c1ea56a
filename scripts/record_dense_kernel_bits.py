"""Records the bits libpgo.so returns on the cases of tests/dense_bits_cases.py: the dense Cholesky solve (csrc/pgo_dense.hip) and the blocked Gauss-Jordan inverse
(csrc/pgo_kernels.hip).  Run once on the GPU:
    python scripts/record_dense_kernel_bits.py [out]          (default out: tests/golden/dense_kernel_bits.json)
Per case the file holds the sha256 of the input bytes and of each output's bytes.  tests/test_gpu_dense_bits.py compares the library's outputs with the file bit for bit,
so a change that alters the bits of the factor, the sweeps or the inverse on purpose re-records with this script; any other change leaves the file alone.  Both paths
promise equal bits between runs: record twice and compare the two files before trusting one.  The script uses the Python API only (capi.Problem), so it runs unchanged
on an older commit's build."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import dense_bits_cases as cases      # noqa: E402


def main(out_path):
    rec = {"cases": {}}
    for name in cases.CASE_NAMES:
        rec["cases"][name] = cases.digests(name)
        print("%-28s %d outputs" % (name, len(rec["cases"][name]["outputs"])), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "dense_kernel_bits.json"))
