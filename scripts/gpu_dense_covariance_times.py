"""Marginal pose covariances from the dense Cholesky factor: time per request.  Run once on the GPU:
    python scripts/gpu_dense_covariance_times.py > profiles/dense_covariance_times.txt
  * session-structured graphs (those of scripts/gpu_dense_cholesky_times.py) of 200, 600 and 1024 keyframes at their initial state; requests: the last keyframe's block
    alone, and the diagonal blocks of all keyframes;
  * kernels: pgo_dense_spd_covariance's avg_ms (HIP events around the right-hand sides, the factorisation, the substitutions and the Gram launch — exactly
    pgo_pose_covariance's launches but for the matrix's build and scatter) on the handle's own undamped reduced matrix, average of 3 after one untimed call; next to it pgo_dense_spd_solve's avg_ms on the same matrix (the
    factorisation and the two sweeps of one dense LM step);
  * call: wall-clock of pgo_pose_covariance itself (linearisation, system build, scatter, factor, covariance, read-back), the fastest of 3 after one untimed call.
Nothing here is a pass/fail number."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from solve_keyframe_pose_graph_amd import capi, graphgen      # noqa: E402
from tests import dense_cov_ref as ref      # noqa: E402
from tests import util      # noqa: E402

print("library: %s" % capi.build_info()[0])
print("milliseconds; kernels = right-hand sides + factor + substitutions + Gram (HIP events), call = pgo_pose_covariance (wall clock), factor + sweeps = pgo_dense_spd_solve on the same matrix")
print("%-6s %6s %9s | %-14s %6s %9s %10s %10s | %14s" % ("graph", "n", "launches", "request", "pairs", "rhs rows", "kernels", "call", "factor+sweeps"))
for N in (200, 600, 1024):
    g = graphgen.generate(N, N // 5, odom_f_max=5, apply_yaw_weight=1, seed=5, **dict(graphgen._SMALL, turn_deg_per_keyframe=2.0))
    q, t, s = util.initial_state(g, True)
    P = util.pgo_problem(g, True, linear_solver=capi.LINEAR_PCG_BLOCK_JACOBI)
    P.evaluate(q, t, s, want_residuals=False, want_gradient=False)
    A = ref.handle_matrix(P, g, True, np.ones(N, bool))
    n = (6 * N + 63) // 64 * 64
    K = capi.Problem()
    K.dense_spd_solve(A, np.ones(6 * N))
    _, ms_solve = K.dense_spd_solve(A, np.ones(6 * N), launches=3)
    for name, pairs in (("last keyframe", [(N - 1, N - 1)]), ("all diagonals", [(a, a) for a in range(N)])):
        K.dense_spd_covariance(A, pairs)
        _, ms = K.dense_spd_covariance(A, pairs, launches=3)
        P.pose_covariance(q, t, s, pairs)
        wall = []
        for _ in range(3):
            t0 = time.perf_counter()
            P.pose_covariance(q, t, s, pairs)
            wall.append((time.perf_counter() - t0) * 1e3)
        nodes = len({a for pr in pairs for a in pr})
        rows = (6 * nodes + 63) // 64 * 64
        k0 = 6 * min(a for pr in pairs for a in pr) // 64
        launches = 1 + 2 * (n // 64 - 1) + 1 + 2 * (n // 64 - k0) - 1 + 1
        print("S%-5d %6d %9d | %-14s %6d %9d %10.3f %10.3f | %14.3f" % (N, n, launches, name, len(pairs), rows, ms, min(wall), ms_solve), flush=True)
    K.close()
    P.close()
