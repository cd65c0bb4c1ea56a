"""Records the bits pgo_pose_covariance and pgo_dense_spd_covariance return on the cases of tests/pose_cov_cases.py.  Run once on the GPU:
    python scripts/record_pose_covariance_bits.py [out]          (default out: tests/golden/pose_covariance_bits.json)
Each 6 x 6 block is stored as 36 float.hex() strings, row-major, beside the pgo_build_info hash of the library that computed it.
tests/test_gpu_dense_covariance.py compares the library's blocks with the file bit for bit, so a change that alters the bits of K1, K2, the system build, the
factorisation or the covariance launches on purpose re-records with this script; any other change leaves the file alone.  The script uses the Python API only
(capi.Problem.dense_spd_covariance, pose_covariance), so it runs unchanged on an older commit's build."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from solve_keyframe_pose_graph_amd import capi      # noqa: E402
from tests import pose_cov_cases as cases      # noqa: E402


def main(out_path):
    rec = {"library": capi.build_info()[0], "cases": {}}
    for name in cases.CASES:
        cov = cases.run(name)["pose"]
        rec["cases"][name] = [[float(v).hex() for v in blk.reshape(-1)] for blk in cov]
        print("%-16s %4d blocks" % (name, len(cov)), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "pose_covariance_bits.json"))
