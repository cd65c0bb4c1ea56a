#!/usr/bin/env python3
"""One linearisation through sparse_cholesky.Graph (pgo_sparse_graph: the companion library's own kernels) against the same through a handle's hooks
(sparse_cholesky.handle_callbacks: pgo_evaluate + pgo_get_normal_blocks, what solve_exact pays per accepted step).

    python scripts/gpu_sparse_graph_times.py [out]          (default out: profiles/sparse_graph_times.txt)

A linearisation = evaluate with a gradient (no residuals) + normal_blocks, both called as the C callbacks pgo_sparse_lm_solve calls, on preallocated host arrays; wall clock,
the fastest of 5 after one warm-up call.  Of the Graph also the HIP-event times of pgo_sparse_graph_last_times, and the same graph with yaw/pitch/roll-weighted loop
closures (gains 4 / 10 / 10), which a handle cannot hold.  Graphs: tests/precond_cases' tl600 and graphgen.generate(N, N // 10, odom_f_max=5, seed=7) at 1100, 3000 and
10000 keyframes, switchable loop closures.  Every graph runs in a child process under its own time limit; after a child that fails nothing more is run.  No threshold:
97 - 99 % of an exact step is the factor and the sweeps (profiles/sparse_lm_times.txt)."""
import ctypes as C
import hashlib
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [("tl600", 120), ("g1100", 120), ("g3000", 180), ("g10000", 300)]      # name, seconds
REPEAT = 5


def graph_of(name):
    from solve_keyframe_pose_graph_amd import graphgen
    if name == "tl600":
        from tests import precond_cases as pc
        return pc.graph("tl600")
    N = int(name[1:])
    return graphgen.generate(N, N // 10, odom_f_max=5, seed=7)


def fastest(cb, user, q, t, s, N, S, E, Es):
    import numpy as np
    dp = C.POINTER(C.c_double)
    P = lambda a: a.ctypes.data_as(dp) if a.size else None
    cost, grad = C.c_double(0), np.zeros(6 * N + S)
    out = [np.zeros(36 * N), np.zeros(6 * N), np.zeros(36 * E), np.zeros(12 * Es), np.zeros(Es), np.zeros(Es)]

    def once():
        t0 = time.perf_counter()
        rc = cb.evaluate(user, P(q), P(t), P(s), N, S, C.cast(C.byref(cost), dp), None, P(grad))
        rc = rc or cb.normal_blocks(user, *[P(a) for a in out])
        if rc != 0:
            raise RuntimeError("a callback failed: %d" % rc)
        return (time.perf_counter() - t0) * 1e3
    once()
    return min(once() for _ in range(REPEAT)), cost.value


def case(name):
    import numpy as np
    from solve_keyframe_pose_graph_amd import sparse_cholesky as sc
    from tests import util
    g = graph_of(name)
    q, t, s = util.initial_state(g, True)
    q, t, s = np.ascontiguousarray(q.reshape(-1)), np.ascontiguousarray(t.reshape(-1)), np.ascontiguousarray(s)
    N, S, E, Es = g.n_poses, g.n_loops, g.n_odom + g.n_loops, g.n_loops
    row = "%-7s %6d %7d |" % (name, N, E + len(g.reg_node))
    for gains in (None, sc.REFERENCE_YPR_GAINS):
        G = sc.Graph.from_pose_graph(g, True, loop_gains=gains)
        cb, user = G.lm_callbacks()
        ms, cost = fastest(cb, user, q, t, s, N, S, E, Es)
        G.evaluate(q, t, s, want_residuals=False)
        tm = G.last_times()
        row += " %8.3f  %6.3f %6.3f %6.3f %6.3f |" % (ms, tm["upload_ms"], tm["blocks_ms"], tm["nodes_ms"], tm["download_ms"])
        if gains is None:
            cost_graph = cost
        G.close()
    Pb = util.pgo_problem(g, True)
    ms_handle, cost_handle = fastest(sc.handle_callbacks(Pb), None, q, t, s, N, S, E, Es)
    Pb.close()
    assert abs(cost_handle - cost_graph) <= 1e-12 * cost_handle, (cost_handle, cost_graph)
    print("ROW " + row + " %8.3f" % ms_handle)


def main(out_path):
    with open(os.path.join(ROOT, "solve_keyframe_pose_graph_amd", "libpgo_sparse.so"), "rb") as f:
        sha = hashlib.sha256(f.read()).hexdigest()
    lines = ["library: %s (libpgo_sparse.so)" % sha,
             "milliseconds of ONE linearisation (evaluate with a gradient + normal_blocks, called as pgo_sparse_lm_solve's callbacks on host arrays): wall clock, the fastest of %d;" % REPEAT,
             "events: HIP events of pgo_sparse_graph_last_times — upload of the state, block kernel + cost reduction, node kernel, download of cost and gradient",
             "graph     nodes  blocks |   Graph: wall  upload blocks  nodes downld |  Graph, yaw/pitch/roll loops: the same   | handle: wall"]
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
    return 0 if len(lines) == 4 + len(CASES) and not any("child process" in ln for ln in lines) else 1


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--case":
        case(sys.argv[2])
    else:
        sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sparse_graph_times.txt")))
