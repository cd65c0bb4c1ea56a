"""The dense Cholesky solver against the default PCG, time per LM system, and its kernels alone.  Run once on the GPU:
    python scripts/gpu_dense_cholesky_times.py > profiles/dense_cholesky_times.txt
  * session-structured graphs (f = 1..5 odometry with yaw weights, one loop closure per 5 keyframes, 2-degree turns) of 200 - 1024 keyframes, 10-iteration solves with the
    tolerances off so that all ten steps run: per LM system seconds_system + seconds_pcg (median over the steps of the second of two solves), linear_solver = 2 against the
    default options;
  * pgo_dense_spd_solve's avg_ms at n = 1536, 3072, 6144 with the implied GFLOP/s (n^3 / 3 for the factor + 2 n^2 for the sweeps).
Nothing here is a pass/fail number."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from solve_keyframe_pose_graph_amd import capi, graphgen      # noqa: E402
from tests import util      # noqa: E402

print("library: %s" % capi.build_info()[0])
print("per LM system: seconds_system + seconds_pcg, median over the steps of a 10-iteration solve (second of two solves on fresh handles), milliseconds")
print("%-6s %10s | %10s %10s %10s | %10s %10s %10s %8s" % ("graph", "keyframes", "dense", "(system)", "(sweeps)", "default", "(system)", "(pcg)", "cg its"))
for n in (200, 400, 600, 800, 1024):
    g = graphgen.generate(n, n // 5, odom_f_max=5, apply_yaw_weight=1, seed=5, **dict(graphgen._SMALL, turn_deg_per_keyframe=2.0))
    q, t, s = util.initial_state(g, True)
    row = []
    for kw in (dict(linear_solver=capi.LINEAR_DENSE_CHOLESKY), {}):
        for rep in range(2):
            P = util.pgo_problem(g, True, max_num_iterations=10, function_tolerance=0.0, parameter_tolerance=0.0, gradient_tolerance=0.0, **kw)
            _, _, _, sm = P.solve(q, t, s)
            P.close()
        its = [sm.iterations[k] for k in range(1, sm.num_logged)]
        sysm, pcg = np.array([it.seconds_system for it in its]) * 1e3, np.array([it.seconds_pcg for it in its]) * 1e3
        row += [np.median(sysm + pcg), np.median(sysm), np.median(pcg)]
        cg = sm.cg_iterations / max(len(its), 1)
    print("S%-5d %10d | %10.3f %10.3f %10.3f | %10.3f %10.3f %10.3f %8.0f" % (n, n, row[0], row[1], row[2], row[3], row[4], row[5], cg), flush=True)

print()
print("pgo_dense_spd_solve (factor + both sweeps, HIP events, average of 3 after one untimed call)")
P = capi.Problem()
for n in (1536, 3072, 6144):
    rng = np.random.default_rng(n)
    B = rng.standard_normal((n, n // 2))
    A = B @ B.T + np.diag(rng.uniform(1e-3, 1.0, n))
    b = rng.standard_normal(n)
    P.dense_spd_solve(A, b)
    _, ms = P.dense_spd_solve(A, b, launches=3)
    flops = n ** 3 / 3.0 + 2.0 * n * n
    print("n %5d  %8.3f ms  %8.1f GFLOP/s  (%d launches)" % (n, ms, flops / ms * 1e-6, 1 + 2 * (n // 64 - 1) + 2 * (n // 64)), flush=True)
P.close()
