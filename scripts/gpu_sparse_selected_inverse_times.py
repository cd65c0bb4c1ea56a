"""The tile-sparse selected inverse of libpgo_sparse.so (pgo_sparse_chol_selected_inverse / _selected_blocks, sparse_cholesky.covariance_all): its time beside the
factor's, and beside the forward-sweep path asked for the same answer.  Run once on the GPU:
    python scripts/gpu_sparse_selected_inverse_times.py [out]          (default out: profiles/sparse_selected_inverse_times.txt)
  * the graphs of scripts/gpu_sparse_cholesky_times.py: session-structured graphs of 200, 600 and 1024 keyframes, graphgen.generate(N, N // 10, odom_f_max=5, seed=7) at
    1100, 3000 and 10000 keyframes; each under natural and under reverse Cuthill-McKee order;
  * HIP-event milliseconds (pgo_sparse_chol_last_ms), the fastest of 3: the factor (fill included), the selected inverse, the gather of all N + n_rel + n_sw blocks
    covariance_all asks for; launches and tile products of the selected inverse; `call`: wall clock of sparse_cholesky.covariance_all itself (linearisation, normal
    blocks to the host, reduction, symbolic phase, allocation, factor, selected inverse, gather, the switch quantities on the host), the fastest of 3 after one untimed call;
  * g1100 and g3000: the way to every keyframe's marginal without the selected inverse — sparse_cholesky.covariance for all (i, i) pairs, which deals them out in
    runs of PGO_SPARSE_MAX_GROUPS / 2 keyframes per pgo_sparse_chol_inverse_blocks — its events (factor + blocks) and its wall clock, once; and the largest scaled
    difference between the two answers' diagonal blocks.
Every graph runs in a child process of its own under a time limit of its own; a child that fails ends the run.  Nothing here is a pass/fail number."""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [("S200", 120), ("S600", 120), ("S1024", 180), ("g1100", 240), ("g3000", 420), ("g10000", 540)]      # name, seconds
MANY_CALLS = ("g1100", "g3000")
HEADER = "%-7s %6s %-8s | %7s %9s | %9s %9s %8s | %8s %9s | %9s | %12s %12s %10s" % ("graph", "n", "order", "tiles L", "MB of Z", "factor", "selected", "gather", "launches", "products", "call",
                                                                                    "sweeps: ms", "sweeps: call", "difference")


def fastest(call, repeat=3):
    call()
    wall = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
    return min(wall)


def one_case(name):
    from solve_keyframe_pose_graph_amd import graphgen
    from solve_keyframe_pose_graph_amd import sparse_cholesky as sc
    from tests import util
    N = int(name[1:])
    if name[0] == "S":
        g = graphgen.generate(N, N // 5, odom_f_max=5, apply_yaw_weight=1, seed=5, **dict(graphgen._SMALL, turn_deg_per_keyframe=2.0))
    else:
        g = graphgen.generate(N, N // 10, odom_f_max=5, seed=7)
    q, t, s = util.initial_state(g, True)
    P = util.pgo_problem(g, True)
    ed = sc.Edges.from_graph(g, True)
    P.evaluate(q, t, s, want_residuals=False)
    diag, _, off, c, hss, _ = P.normal_blocks()
    free = np.ones(N, np.uint8)
    hi, lo, sd, sb = sc.reduce_normal_blocks(N, free, diag, off, c, hss, ed.rel_c1, ed.rel_c2, ed.sw_c1, ed.sw_c2)
    na, nb = sc.all_block_requests(N, ed)
    n = (6 * N + 63) // 64 * 64
    for ordering, label in ((sc.ORDER_NATURAL, "natural"), (sc.ORDER_RCM, "rcm")):
        F = sc.SparseCholesky(N, free, hi, lo, ordering)
        info, _ = F.info()
        F.factor(sd, sb)
        factor, selected, gather = [], [], []
        for _ in range(3):
            F.factor(sd, sb); factor.append(F.last_ms())
        F.selected_inverse()
        for _ in range(3):
            F.selected_inverse(); selected.append(F.last_ms())
        sel = F.selected_info()
        F.selected_blocks(na, nb)
        for _ in range(3):
            F.selected_blocks(na, nb); gather.append(F.last_ms())
        F.close()
        res = sc.covariance_all(P, ed, q, t, s, ordering=ordering)
        call = fastest(lambda: sc.covariance_all(P, ed, q, t, s, ordering=ordering))
        sweeps_ms = sweeps_call = diff = float("nan")
        if name in MANY_CALLS:
            tm = {}
            t0 = time.perf_counter()
            cov = sc.covariance(P, ed, q, t, s, [(i, i) for i in range(N)], ordering=ordering, timings=tm)
            sweeps_call = (time.perf_counter() - t0) * 1e3
            sweeps_ms = tm["factor_ms"] + tm["blocks_ms"]
            cov = np.stack(cov)
            d = np.sqrt(np.diagonal(cov, axis1=1, axis2=2))
            diff = float((np.abs(cov - res.pose) / (d[:, :, None] * d[:, None, :])).max())
        print("ROW %-7s %6d %-8s | %7d %9.1f | %9.3f %9.3f %8.3f | %8d %9d | %9.1f | %12.1f %12.1f %10.1e"
              % (name, n, label, info["l_tiles"], sel["bytes"] / 1e6, min(factor), min(selected), min(gather), sel["launches"], sel["tile_products"], call, sweeps_ms, sweeps_call, diff), flush=True)
    P.close()


def main(out_path):
    from solve_keyframe_pose_graph_amd import capi
    lines = ["library: %s (libpgo.so; libpgo_sparse.so is built beside it from csrc/pgo_sparse.hip)" % capi.build_info()[0],
             "milliseconds; factor, selected (inverse), gather (of the N + n_rel + n_sw blocks of covariance_all): HIP events, the fastest of 3; call: wall clock of sparse_cholesky.covariance_all; "
             "sweeps: sparse_cholesky.covariance for all (i, i), 32 keyframes per pgo_sparse_chol_inverse_blocks — its events (factor + blocks) and its wall clock, once; "
             "difference: the largest scaled difference of the two answers' diagonal blocks", HEADER]
    print("\n".join(lines), flush=True)
    for name, seconds in CASES:
        out = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), "--case", name], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        rows = [ln[4:] for ln in out.stdout.splitlines() if ln.startswith("ROW ")]
        print("\n".join(rows), flush=True)
        lines += rows
        if out.returncode != 0:
            print(out.stderr[-3000:], file=sys.stderr)
            lines.append("%s: the child process ended with status %d; nothing after it was run" % (name, out.returncode))
            break
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if lines[-1].count("ended with status") == 0 else 1


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--case":
        one_case(sys.argv[2])
    else:
        sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sparse_selected_inverse_times.txt")))
