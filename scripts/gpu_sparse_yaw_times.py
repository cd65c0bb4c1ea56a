#!/usr/bin/env python3
"""One linearisation and one exact LM step through sparse_cholesky.YawGraph (pgo_sparse_yaw_graph: the 4-DoF graph, 4-row residuals in six-row slots) against the same
through sparse_cholesky.Graph (pgo_sparse_graph with SixDOFError edges on the same keyframe pairs, loop closures as relative-pose edges), in the same process.

    python scripts/gpu_sparse_yaw_times.py [out]          (default out: profiles/sparse_yaw_times.txt)

A linearisation = evaluate with a gradient (no residuals) + normal_blocks, both called as the C callbacks pgo_sparse_lm_solve calls, on preallocated host arrays.  An LM
step = SparseLm.step on those blocks at radius 1e4 (upload, damping + fill, factor, sweeps, back-substitution, download).  Wall clock and HIP events
(pgo_sparse_yaw_graph_last_times / pgo_sparse_graph_last_times; pgo_sparse_lm_last_times), the median of 11 runs after one warm-up run.  Graphs: tests/precond_cases'
tl600 and graphgen.generate(N, N // 10, odom_f_max=5, seed=7) at 1100, 3000 and 10000 keyframes; keyframe 0 constant in the yaw graph, the generator's regulariser in the
other.  Every graph runs in a child process under its own time limit; after a child that fails nothing more is run.  No threshold: the claim is not speed."""
import ctypes as C
import hashlib
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [("tl600", 120), ("g1100", 120), ("g3000", 180), ("g10000", 300)]      # name, seconds
REPEAT = 11


def graph_of(name):
    from solve_keyframe_pose_graph_amd import graphgen
    if name == "tl600":
        from tests import precond_cases as pc
        return pc.graph("tl600")
    N = int(name[1:])
    return graphgen.generate(N, N // 10, odom_f_max=5, seed=7)


def measure(G, q, t, N, E, lists):
    """-> medians: linearisation wall, its four event times, LM step wall, its six event times"""
    import numpy as np
    from solve_keyframe_pose_graph_amd import sparse_cholesky as sc
    dp = C.POINTER(C.c_double)
    P = lambda a: a.ctypes.data_as(dp) if a.size else None
    cb, user = G.lm_callbacks()
    cost, grad = C.c_double(0), np.zeros(6 * N)
    diag, g6, off = np.zeros(36 * N), np.zeros(6 * N), np.zeros(36 * E)
    none = np.zeros(0)
    lin, lin_ev = [], []
    for _ in range(REPEAT + 1):
        t0 = time.perf_counter()
        rc = cb.evaluate(user, P(q), P(t), None, N, 0, C.cast(C.byref(cost), dp), None, P(grad))
        rc = rc or cb.normal_blocks(user, P(diag), P(g6), P(off), None, None, None)
        lin.append((time.perf_counter() - t0) * 1e3)
        if rc != 0:
            raise RuntimeError("a callback failed: %d" % rc)
        tm = G.last_times()
        lin_ev.append([tm[k] for k in sc.GRAPH_TIMES])
    F = sc.SparseCholesky(N, lists["in_system"], lists["pair_hi"], lists["pair_lo"], sc.ORDER_AUTO, G.device_id)
    L = sc.SparseLm(F, lists["node_free"], lists["c1"], lists["c2"], np.zeros(0, np.int32), np.zeros(0, np.int32))
    L.set_scale(diag, none)
    step, step_ev = [], []
    for _ in range(REPEAT + 1):
        t0 = time.perf_counter()
        L.step(diag, g6, off, none, none, none, 1e4)
        step.append((time.perf_counter() - t0) * 1e3)
        tm = L.last_times()
        step_ev.append([tm[k] for k in sc.LM_TIMES])
    tiles = F.info()[0]["l_tiles"]
    L.close(); F.close()
    med = lambda x: np.median(np.array(x[1:]), axis=0)
    return med(lin), med(lin_ev), med(step), med(step_ev), tiles, cost.value


def case(name):
    import numpy as np
    from solve_keyframe_pose_graph_amd import sparse_cholesky as sc
    from tests import util
    g = graph_of(name)
    N, E = g.n_poses, g.n_odom + g.n_loops
    Y, yaw, t, _, _ = sc.YawGraph.from_pose_graph(g)
    ya = measure(Y, np.ascontiguousarray(Y.pack(yaw).reshape(-1)), np.ascontiguousarray(t.reshape(-1)), N, E, Y.edge_lists())
    Y.close()
    G = sc.Graph.from_pose_graph(g, False)
    q, t6, _ = util.initial_state(g, False)
    e = G.edge_lists()
    e["c1"], e["c2"] = e["rel_c1"], e["rel_c2"]
    ga = measure(G, np.ascontiguousarray(q.reshape(-1)), np.ascontiguousarray(t6.reshape(-1)), N, E, e)
    G.close()
    for what, m in (("YawGraph", ya), ("Graph", ga)):
        print("ROW %-7s %6d %6d %-8s | %7.3f  %6.3f %6.3f %6.3f %6.3f | %8.3f  %6.3f %6.3f %8.3f %6.3f %6.3f %6.3f | %5d" % ((name, N, E, what, m[0]) + tuple(m[1]) + (m[2],) + tuple(m[3]) + (m[4],)))


def main(out_path):
    with open(os.path.join(ROOT, "solve_keyframe_pose_graph_amd", "libpgo_sparse.so"), "rb") as f:
        sha = hashlib.sha256(f.read()).hexdigest()
    lines = ["library: %s (libpgo_sparse.so), built by _build.build_libpgo_sparse: hipcc --offload-arch=gfx950 -O3 -ffp-contract=on" % sha,
             "milliseconds, the median of %d runs after a warm-up run, YawGraph (QinFourDOFWeightError, 4 rows) and Graph (SixDOFError, 6 rows) on the same keyframe pairs in one process" % REPEAT,
             "linearisation: evaluate with a gradient + normal_blocks as pgo_sparse_lm_solve's callbacks; events: upload of the state, block kernel + cost reduction, node kernel, download",
             "LM step: pgo_sparse_lm_step at radius 1e4; events: upload, damping + fill + right-hand side, factor, sweeps, back-substitution + model, download",
             "graph     nodes  edges object   | lin: wall  upload blocks  nodes downld | step: wall  upload   fill   factor sweeps backsb downld | tiles of L"]
    head = len(lines)
    for name, seconds in CASES:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=seconds)
        lines += [ln[4:] for ln in out.stdout.splitlines() if ln.startswith("ROW ")]
        if out.returncode != 0:
            print(out.stderr[-3000:], file=sys.stderr)
            lines.append("%s: the child process ended with status %d; nothing after it was run" % (name, out.returncode))
            break
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0 if len(lines) == head + 2 * len(CASES) and not any("child process" in ln for ln in lines) else 1


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--case":
        case(sys.argv[2])
    else:
        sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sparse_yaw_times.txt")))
