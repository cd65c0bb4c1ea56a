"""Records the bits libpgo.so returns on the cases of tests/pcg_bits_cases.py: the iterates x_k of every form of the PCG iteration (block-Jacobi, the two-level method and
the multigrid, each classic, single-reduction and block-CSR; csrc/pgo_kernels.hip, csrc/pgo_mg_kernels.hpp, csrc/pgo_pcg_ops.hpp).  Run once on the GPU:
    python scripts/record_pcg_kernel_bits.py [out]          (default out: tests/golden/pcg_kernel_bits.json)
Per case the file holds the sha256 of the input bytes and of each output's bytes.  tests/test_gpu_pcg_bits.py compares the library's outputs with the file bit for bit,
so a change that alters an iterate's bits on purpose re-records with this script; any other change leaves the file alone.  Every form promises equal bits between
runs: record twice and compare the two files before trusting one.  The script uses the Python API only (capi.Problem through tests/precond_child.py), so it runs
unchanged on an older commit's build."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import pcg_bits_cases as cases      # noqa: E402


def main(out_path):
    rec = {"cases": {}}
    for name in cases.CASE_NAMES:
        rec["cases"][name] = cases.digests(name)
        print("%-44s %d outputs" % (name, len(rec["cases"][name]["outputs"])), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "pcg_kernel_bits.json"))
