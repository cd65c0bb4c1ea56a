"""Covariance blocks of pose and switch parameters (pgo_covariance): time per request.  Run once on the GPU:
    python scripts/gpu_param_covariance_times.py [out]          (default out: profiles/param_covariance_times.txt)
  * session-structured graphs (those of scripts/gpu_dense_covariance_times.py) of 200, 600 and 1024 keyframes with N / 5 switchable loop closures, at their initial
    state; requests: (a) the last keyframe's block alone, (b) the diagonal blocks of all keyframes, (c) the variances of all switches;
  * kernels: pgo_dense_spd_param_covariance's avg_ms (HIP events around the right-hand sides, the FACTORISATION, the substitutions and the Gram launch — pgo_covariance's
    launches after the matrix is in place) on the handle's own undamped reduced matrix and switch columns, average of 3 after one untimed call; beside it
    pgo_dense_spd_covariance's avg_ms (the same launches through the pose-only hook: a second measurement of the same thing) for (a) and (b);
  * call: wall clock of pgo_covariance itself (linearisation, the matrix, factor, covariance, read-back), the fastest of 3 after one untimed call, on a block-CSR handle
    (linear_solver = 0: build_rows + scatter) and on a matrix-free handle (the default: J1^T J2 per edge, host plan, one scatter); beside it pgo_pose_covariance (the same routine through its own entry point) on the
    block-CSR handle for (a) and (b).  The difference of the two pgo_covariance columns is what the matrix-free assembly costs more (or less) than build_rows + scatter.
Nothing here is a pass/fail number."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from solve_keyframe_pose_graph_amd import capi, graphgen      # noqa: E402
from tests import dense_cov_ref as ref      # noqa: E402
from tests import util      # noqa: E402


def fastest(call, repeat=3):
    call()
    wall = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
    return min(wall)


def main(out_path):
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("library: %s" % capi.build_info()[0])
    emit("milliseconds; kernels = right-hand sides + factor + substitutions + Gram (HIP events; pose: the same launches through pgo_dense_spd_covariance), call = wall clock of the entry point")
    emit("%-6s %6s %5s | %-14s %6s %9s | %9s %9s | %12s %12s %12s" % ("graph", "n", "sw", "request", "pairs", "rhs rows", "kernels", "pose", "call csr", "call mf", "pose call"))
    for N in (200, 600, 1024):
        g = graphgen.generate(N, N // 5, odom_f_max=5, apply_yaw_weight=1, seed=5, **dict(graphgen._SMALL, turn_deg_per_keyframe=2.0))
        S = g.n_loops
        q, t, s = util.initial_state(g, True)
        P = util.pgo_problem(g, True, linear_solver=capi.LINEAR_PCG_BLOCK_JACOBI)
        M = util.pgo_problem(g, True)
        P.evaluate(q, t, s, want_residuals=False, want_gradient=False)
        A = ref.handle_matrix(P, g, True, np.ones(N, bool))
        _, _, _, c, hss, _ = P.normal_blocks()
        nodes = np.stack([g.loop_c1, g.loop_c2], axis=1).astype(np.int32)
        n = (6 * N + 63) // 64 * 64
        K = capi.Problem()
        requests = (("last keyframe", [(N - 1, N - 1)], True), ("all keyframes", [(a, a) for a in range(N)], True), ("all switches", [(N + e, N + e) for e in range(S)], False))
        for name, pairs, pose in requests:
            K.dense_spd_param_covariance(A, nodes, c, hss, pairs)
            _, ms = K.dense_spd_param_covariance(A, nodes, c, hss, pairs, launches=3)
            ms_pose = wall_pose = float("nan")
            if pose:
                K.dense_spd_covariance(A, pairs)
                _, ms_pose = K.dense_spd_covariance(A, pairs, launches=3)
                wall_pose = fastest(lambda: P.pose_covariance(q, t, s, pairs))
            wall_csr = fastest(lambda: P.covariance(q, t, s, pairs))
            wall_mf = fastest(lambda: M.covariance(q, t, s, pairs))
            rows = sum(6 if i < N else 1 for i in {a for pr in pairs for a in pr})
            rows = (rows + 63) // 64 * 64
            emit("S%-5d %6d %5d | %-14s %6d %9d | %9.3f %9.3f | %12.3f %12.3f %12.3f" % (N, n, S, name, len(pairs), rows, ms, ms_pose, wall_csr, wall_mf, wall_pose))
        assert M.matrix_free_tiles()["n_tiles"] > 0
        K.close(); P.close(); M.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "param_covariance_times.txt"))
