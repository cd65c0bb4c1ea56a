"""The tile-sparse Cholesky companion library (libpgo_sparse.so): time of the factor, of one solve and of the last keyframe's covariance.  Run once on the GPU:
    python scripts/gpu_sparse_cholesky_times.py [out]          (default out: profiles/sparse_cholesky_times.txt)
  * session-structured graphs (those of scripts/gpu_dense_covariance_times.py) of 200, 600 and 1024 keyframes, with Problem.dense_spd_solve (factor + sweeps of the dense
    solver on the same matrix, HIP events) and Problem.covariance (wall clock) beside them;
  * graphgen.generate(N, N // 10, odom_f_max=5, seed=7) at 1100, 3000 and 10000 keyframes, above the dense limit;
  * every graph under natural and under reverse Cuthill-McKee order: tiles of L, bytes, and HIP-event milliseconds (pgo_sparse_chol_last_ms) of factor (fill included),
    of one solve (2 nt launches) and of covariance(last keyframe) = factor + forward sweep of six rows + Gram; `call`: wall clock of sparse_cholesky.covariance itself
    (linearisation, normal blocks to the host, reduction, symbolic phase, allocation, factor, blocks), the fastest of 3 after one untimed call.
Every graph runs in a child process of its own under a time limit of its own; a child that fails ends the run.  Nothing here is a pass/fail number."""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [("S200", 120), ("S600", 120), ("S1024", 180), ("g1100", 180), ("g3000", 240), ("g10000", 420)]      # name, seconds
HEADER = "%-7s %6s %-8s | %7s %9s | %9s %9s %11s %10s | %12s %12s" % ("graph", "n", "order", "tiles L", "MB", "factor", "solve", "cov(last)", "call", "dense f+s", "dense call")


def fastest(call, repeat=3):
    call()
    wall = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
    return min(wall)


def one_case(name):
    from solve_keyframe_pose_graph_amd import capi, graphgen
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
    b = np.random.default_rng(1).standard_normal(6 * N)
    n = (6 * N + 63) // 64 * 64
    dense_ms = dense_call = float("nan")
    if N <= capi.DENSE_MAX_KEYFRAMES:
        A = np.zeros((6 * N, 6 * N))
        for i in range(N):
            A[6 * i:6 * i + 6, 6 * i:6 * i + 6] = sd[i]
        for k, (x, y) in enumerate(zip(hi, lo)):
            A[6 * x:6 * x + 6, 6 * y:6 * y + 6] = sb[k]; A[6 * y:6 * y + 6, 6 * x:6 * x + 6] = sb[k].T
        K = capi.Problem()
        K.dense_spd_solve(A, b)
        _, dense_ms = K.dense_spd_solve(A, b, launches=3)
        K.close()
        dense_call = fastest(lambda: P.covariance(q, t, s, [(N - 1, N - 1)]))
    for ordering, label in ((sc.ORDER_NATURAL, "natural"), (sc.ORDER_RCM, "rcm")):
        F = sc.SparseCholesky(N, free, hi, lo, ordering)
        info, _ = F.info()
        F.factor(sd, sb)
        factor = []
        for _ in range(3):
            F.factor(sd, sb); factor.append(F.last_ms())
        F.solve(b)
        solve = []
        for _ in range(3):
            F.solve(b); solve.append(F.last_ms())
        F.close()
        tm = {}
        cov = []
        sc.covariance(P, ed, q, t, s, [(N - 1, N - 1)], ordering=ordering)
        for _ in range(3):
            sc.covariance(P, ed, q, t, s, [(N - 1, N - 1)], ordering=ordering, timings=tm); cov.append(tm["factor_ms"] + tm["blocks_ms"])
        call = fastest(lambda: sc.covariance(P, ed, q, t, s, [(N - 1, N - 1)], ordering=ordering))
        print("ROW %-7s %6d %-8s | %7d %9.1f | %9.3f %9.3f %11.3f %10.1f | %12.3f %12.3f" % (name, n, label, info["l_tiles"], info["bytes"] / 1e6, min(factor), min(solve), min(cov), call, dense_ms, dense_call), flush=True)
    P.close()


def main(out_path):
    from solve_keyframe_pose_graph_amd import capi
    lines = ["library: %s (libpgo.so; libpgo_sparse.so is built beside it from csrc/pgo_sparse.hip)" % capi.build_info()[0],
             "milliseconds; factor, solve, cov(last) = factor + six-row forward sweep + Gram: HIP events, the fastest of 3; call: wall clock of sparse_cholesky.covariance(last keyframe); "
             "dense f+s: pgo_dense_spd_solve's events on the same matrix; dense call: wall clock of pgo_covariance(last keyframe)", HEADER]
    print("\n".join(lines), flush=True)
    for name, seconds in CASES:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=seconds)
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
        sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sparse_cholesky_times.txt")))
