#!/usr/bin/env python3
"""bench.py — headline benchmark of the hot path (BASELINE.json): Levenberg-Marquardt iterations/s of the
MI355X-native pose-graph solver on the synthetic 100k-pose / 300k-edge switchable-constraint SE(3) graph (C3).

  python bench.py --gpus N --steps K --warmup W
  (N > 1: python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ... bench.py --gpus N ...)

A "step" is ONE trust-region LM iteration of pgo_lm_step: lm-diagonal, Schur-reduced system build, block-Jacobi PCG
solve, model-cost change, candidate Plus, candidate cost (K1 cost-only) and — when the step is accepted —
re-linearisation (K1 + K2).  Inputs are resident in HBM when the timed region starts (pgo_solve_begin is outside it).
N GPUs: weak scaling — the graph is N x C3 (N*100k poses / N*300k edges), edges sharded contiguously across ranks,
one RCCL all-reduce per CG matvec inside libpgo; `value` = LM iterations/s x N (C3-sized graph-iterations per second).

A plain run sets up, warms up, times the K steps and prints the line (`value`, `ms_per_step`, the timed solve's chi2 against the
independent CPU trajectory).  `--full` adds everything that takes runs of its own: the per-kernel / `roofline` figures (HIP events on
the library's own stream), the leg including transfers, K1 out of cache, Ceres' decision rule, the solve to convergence, `cpu_baseline`
(the CPU oracle = a restatement of the reference's Ceres path, timed on the host cores on a bounded sample; rank 0, N = 1 only) and,
with several ranks, the `c5_strong` leg.

`--dump-outputs DIR` writes what the timed path hands its caller after the last timed step (dump_outputs) as DIR/<name>.npy.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

HBM_PEAK_GBS = 8000.0   # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
C3_POSES, C3_LOOPS, C3_EDGES = 100000, 100003, 300000


def probe_real_ceres():
    """The reference's real CPU path needs Ceres + Eigen (reference CMakeLists.txt:22-23).  If this host has them, oracle/ceres_bench.cpp (own
    functors, real ceres::Solve) is built and run (run_real_ceres); report what was found so that the baseline's kind is never mistaken."""
    import glob
    hits = [p for pat in ("/usr/include/ceres/ceres.h", "/usr/local/include/ceres/ceres.h", "/opt/*/include/ceres/ceres.h") for p in glob.glob(pat)]
    eig = [p for pat in ("/usr/include/eigen3/Eigen/Core", "/usr/local/include/eigen3/Eigen/Core", "/usr/include/Eigen/Core") for p in glob.glob(pat)]
    return {"ceres_header": hits[0] if hits else None, "eigen_header": eig[0] if eig else None}


def run_real_ceres(sample_poses, max_iters):
    """Builds and runs oracle/ceres_bench (own functor restatement + the REAL ceres::Solve) when this host has Ceres and Eigen3; None otherwise."""
    import subprocess
    pr = probe_real_ceres()
    if not (pr["ceres_header"] and pr["eigen_header"]):
        return None
    try:
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-s", "ceres_bench"], timeout=600)
        exe = os.path.join(ROOT, "oracle", "ceres_bench")
        if not os.path.exists(exe):
            return {"error": "ceres_bench was not built"}
        res = {}
        for label, nt in (("one_thread", 1), ("all_cores", min(os.cpu_count() or 1, 32))):
            out = subprocess.check_output([exe, str(sample_poses), str(sample_poses), "2", "3", str(max_iters), str(nt)], timeout=900)
            res[label] = json.loads(out.decode().strip().splitlines()[-1])
        return res
    except Exception as e:
        return {"error": repr(e)}


def measured_c3():
    """The one full-size measurement of the CPU port on C3 (hours of CPU: not repeated inside the driver's bench run)"""
    for name in ("r05_cpu_c3_full_gpubox.json", "r04_cpu_c3_full.json"):      # round 5: the first LM iteration on a GPU box's own host (EPYC 9575F); round 4: three iterations in the build container
        try:
            with open(os.path.join(ROOT, "profiles", name)) as f:
                d = json.load(f)
            return {"value": d["lm_iterations_per_second"], "unit": "LM iters/s", "cores": 1, "kind": "port", "seconds_per_lm_iteration": d["seconds_per_lm_iteration"], "lm_iterations": d["lm_iterations"],
                    "seconds_linear_solver": d["seconds_linear_solver"], "cholesky_fill_blocks": d["cholesky_fill_blocks"], "host_cpu": d.get("host_cpu"), "file": "profiles/" + name,
                    "note": "measured at full size on %s (%s); static (not re-measured in this run)" % (d.get("machine") or "the GPU box's host", d.get("host_cpu") or "?")}
        except Exception:
            continue
    return None


def c3_direct_solve_estimate(full):
    try:
        with open(os.path.join(ROOT, "profiles", "r06_cpu_cholesky_flops.json")) as f:
            c3 = json.load(f)["C3"]
        tf = c3["cholesky_flops"] * 1e-12
        out = {"cholesky_tflop_per_lm_iteration": tf, "cholesky_fill_blocks": c3["cholesky_fill_blocks"], "ordering": "approximate minimum degree (oracle/sparse_chol.hpp); a nested-dissection ordering typically needs 2-3x fewer flops on mesh-like graphs",
               "source": "profiles/r06_cpu_cholesky_flops.json (symbolic factorisation of the full C3 normal matrix, exact)"}
        if full and full.get("seconds_linear_solver"):
            out["port_measured_gflops_per_s"] = c3["cholesky_flops"] * 1e-9 / full["seconds_linear_solver"]
        out["estimates_not_measurements"] = {
            "one_core_supernodal_at_30_to_60_gflops": {"seconds_per_lm_iteration": [tf * 1e3 / 60.0, tf * 1e3 / 30.0], "lm_iters_per_s": [30.0 / (tf * 1e3), 60.0 / (tf * 1e3)]},
            "64_cores_at_2_tflops_aggregate": {"seconds_per_lm_iteration": tf / 2.0, "lm_iters_per_s": 2.0 / tf},
            "note": "what Ceres + CHOLMOD (supernodal, BLAS-3) would need for the factorisation alone at plausible rates on this host; neither can be built here, so these are arithmetic on an exact flop count, not runs"}
        return out
    except Exception as e:
        return {"error": repr(e)}


def cpu_baseline(sample_poses, max_iters, budget_s):
    """Times the oracle (oracle/pgo_oracle.cpp: Jet autodiff + Ceres-style LM + exact block-sparse Cholesky) on a C3-structured sample that fits
    the time budget: once with 1 thread (faithful: the reference never sets num_threads, Ceres default 1) and once with the residual blocks
    evaluated on all host cores (Ceres' num_threads; the sparse Cholesky stays serial, as a simplicial CHOLMOD is)."""
    from oracle import binding as ob
    from solve_keyframe_pose_graph_amd import graphgen
    from tests import util
    g = graphgen.generate(sample_poses, sample_poses, odom_f_max=2, seed=3)
    O = util.oracle_problem(g, True)
    q, t, s = util.initial_state(g, True)
    edges = g.n_odom + g.n_loops
    ncpu = os.cpu_count() or 1
    nthreads = min(ncpu, 32)     # beyond ~32 threads the 72k residual blocks of the sample are too little work per thread (256 threads: 3x slower than 1)
    runs = {}
    for label, nt in (("one_thread", 1), ("all_cores", nthreads)):
        t0 = time.time()
        # no early stop: the same fixed iteration budget the GPU leg times
        opt = ob.default_options(max_num_iterations=max_iters, function_tolerance=0.0, parameter_tolerance=0.0, gradient_tolerance=0.0, num_threads=nt)
        _, _, _, sm = O.solve(q, t, s, opt)
        wall = time.time() - t0
        iters = max(1, sm.num_iterations)
        runs[label] = dict(ips=iters / sm.seconds_total, wall=wall, lin=sm.seconds_linear_solver, jac=sm.seconds_jacobian, fill=sm.chol_nnz_blocks, iters=iters,
                           chol_gflops=float(ob.lib().orc_last_cholesky_flops()) * 1e-9)
    one, allc = runs["one_thread"], runs["all_cores"]
    # How the 1-thread time grows with the graph: the same run on half the sample.  The sparse Cholesky's fill grows faster than the edge count on this mesh-like
    # graph, so the LINEAR scaling to 300k edges used for `value` flatters the CPU; the measured exponent and the power-law extrapolation stand next to it.
    growth = None
    try:
        gh = graphgen.generate(sample_poses // 2, sample_poses // 2, odom_f_max=2, seed=3)
        Oh = util.oracle_problem(gh, True)
        qh, th, sh = util.initial_state(gh, True)
        opt = ob.default_options(max_num_iterations=max_iters, function_tolerance=0.0, parameter_tolerance=0.0, gradient_tolerance=0.0, num_threads=1)
        _, _, _, smh = Oh.solve(qh, th, sh, opt)
        eh = gh.n_odom + gh.n_loops
        per_it_full, per_it_half = 1.0 / one["ips"], smh.seconds_total / max(1, smh.num_iterations)
        expo = float(np.log(per_it_full / per_it_half) / np.log(edges / eh))
        growth = {"half_sample_edges": eh, "half_sample_s_per_iteration": per_it_half, "full_sample_s_per_iteration": per_it_full, "fill_blocks_half": int(smh.chol_nnz_blocks), "fill_blocks_full": int(one["fill"]),
                  "time_exponent_vs_edges": expo, "power_law_value_at_300k_edges": 1.0 / (per_it_full * (C3_EDGES / edges) ** expo)}
    except Exception as e:
        growth = {"error": repr(e)}
    # kernel-level companion number on the FULL C3 graph: one residual + Jacobian evaluation of all 300k edges by the oracle's Jet
    # autodiff (what Ceres' evaluator does per linearisation) — the CPU counterpart of K1, no linear algebra involved
    g3 = graphgen.config("C3")
    O3 = util.oracle_problem(g3, True)
    q3, t3, s3 = util.initial_state(g3, True)
    tj = time.time()
    O3.evaluate(q3, t3, s3, want_residuals=False, want_gradient=True)
    jac_ms = 1e3 * (time.time() - tj)
    full = measured_c3()      # the port on the FULL C3 graph, measured on a GPU box's host (static file of an earlier round: 30 minutes of CPU per iteration do not fit this run)
    linear_value = one["ips"] * edges / C3_EDGES
    port_rate = one["chol_gflops"] * one["iters"] / max(one["lin"], 1e-9)      # GFLOP/s of the port's factorisations on the sample
    return {
        # round 6: `value` is the MEASURED full-size figure where one exists; the sample scaled linearly by edges — optimistic for the CPU by two orders of
        # magnitude, the sparse Cholesky being super-linear — stays as a labelled extra
        "value": full["value"] if full and full.get("value") else linear_value,
        "value_is": ("MEASURED on the full C3 graph: %s" % full["note"] + " (" + full["file"] + ")") if full and full.get("value") else "the sample of this run scaled linearly by edges (no full-size measurement on file)",
        "unit": "LM iters/s (C3)",
        "cores": 1,
        "kind": "port",
        "sample": "%d LM iterations of the oracle on a C3-structured %d-pose / %d-edge graph (same generator, seed 3), timed in this run: %.3f LM iters/s on the sample "
                  "(%.2f s, linear solver %.2f s, Jacobians %.2f s, Cholesky fill %d blocks, %.1f GFLOP per factorisation = %.2f GFLOP/s)"
                  % (one["iters"], g.n_poses, edges, one["ips"], one["wall"], one["lin"], one["jac"], one["fill"], one["chol_gflops"], port_rate),
        "sample_iters_per_s": one["ips"],
        "sample_scaled_linearly_by_edges": linear_value,
        "port_cholesky_gflops_per_s": port_rate,
        # the work ANY direct solver with this ordering has to do per LM iteration on the full C3 graph — exact, from the symbolic factorisation (profiles/r06_cpu_cholesky_flops.json,
        # oracle orc_cholesky_symbolic: the fill equals the measured run's 21 857 781 blocks) — and what it means at the rates a supernodal code reaches (ESTIMATES, labelled as such)
        "c3_direct_solve": c3_direct_solve_estimate(full),
        "what_a_supernodal_solver_would_change": "the port's up-looking 6x6-block Cholesky runs at the rate above; a supernodal code (CHOLMOD: BLAS-3 panels) reaches 10-30x that on one core at C3's "
                                                 "fill (21.9 M blocks) — scipy's SuperLU, the one supernodal solver in this image, is 4.7x SLOWER than the port on the 24 000-pose sample "
                                                 "(profiles/r06_cpu_supernodal_crosscheck.json), so it is no better baseline; Ceres + CHOLMOD cannot be built here (reference CMakeLists.txt:22-23)",
        "all_cores": {"value": allc["ips"] * edges / C3_EDGES, "cores": nthreads, "sample_iters_per_s": allc["ips"],
                      "note": "residual blocks / Jacobians on %d OpenMP threads of the host's %d cpus (%.2f s -> %.2f s), sparse Cholesky serial (%.2f s)" % (nthreads, ncpu, one["jac"], allc["jac"], allc["lin"])},
        "c3_jacobian_evaluation_ms": jac_ms,   # CPU (1 thread) residuals + autodiff Jacobians + J^T r of all 300k C3 edges; GPU: roofline.avg_launch_ms
        "host_cpus": ncpu,
        "growth": growth,
        "measured_c3": measured_c3(),   # the port on the FULL C3 graph, measured (not scaled): profiles/r04_cpu_c3_full.json, taken once per round by scripts/cpu_c3_full.py
        "real_ceres_probe": probe_real_ceres(),   # both null: the reference's own CPU path cannot be built on this host -> kind stays "port"
        "real_ceres": run_real_ceres(sample_poses, max_iters),   # oracle/ceres_bench.cpp (functor restatement + real ceres::Solve) where Ceres + Eigen3 exist; null here
    }


DUMP_BYTES_MAX = 64 * 10 ** 6


def dump_outputs(out_dir, q, t, s, summ):
    """--dump-outputs: what a caller of the timed path receives from pgo_solve_end after the last timed step — the state (quaternions
    x, y, z, w and translations per keyframe, one weight per switchable loop) and the summary's costs — as float64 DIR/<name>.npy.  The
    inputs are the same for the same arguments (seeded generator, odometry initial guess), so two builds compare array by array.  Above
    64 MB in all (graphs larger than C3 x 2) the keyframes and the switches are a fixed sample: seed 0, the same for the same graph."""
    n, m = q.size // 4, s.size
    arrays = {"quaternions": q.reshape(n, 4), "translations": t.reshape(n, 3), "switches": s,
              "cost_per_iteration": np.array([summ.iterations[k].cost for k in range(summ.num_logged)]),     # entry 0 = the initial cost
              "final_cost": np.array([summ.final_cost])}
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_BYTES_MAX:
        keep = 0.98 * DUMP_BYTES_MAX / total      # (room for the .npy headers)
        rng = np.random.default_rng(0)
        kp = np.sort(rng.choice(n, int(n * keep), replace=False))
        ks = np.sort(rng.choice(m, int(m * keep), replace=False))
        arrays.update(quaternions=arrays["quaternions"][kp], translations=arrays["translations"][kp], switches=s[ks])
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(a, dtype=np.float64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)     # the reference's LM budget per trigger: max_num_iterations = 10
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--full", action="store_true", help="everything beyond the headline figure as well: per-kernel / roofline timings, the leg including transfers, K1 out of cache, "
                    "Ceres' decision rule, the solve to convergence, the CPU baseline and (several ranks) the c5_strong leg")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps, write what they computed (final state and costs) as DIR/<name>.npy, float64, at most 64 MB")
    ap.add_argument("--cg-tol", type=float, default=None, help="PCG relative tolerance (default: library default)")
    ap.add_argument("--cg-max", type=int, default=None)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-k1-out-of-cache", action="store_true", help="skip the second K1 measurement on a 400k-keyframe graph")
    ap.add_argument("--cpu-sample-poses", type=int, default=24000)
    ap.add_argument("--cpu-iters", type=int, default=5)
    ap.add_argument("--poses-per-gpu", type=int, default=C3_POSES)
    ap.add_argument("--collective", choices=["rccl", "gloo"], default="rccl",
                    help="rccl: libpgo's own RCCL communicator over xGMI (default).  gloo: torch.distributed gloo through pgo_comm_init_custom "
                         "(host staging; lets several ranks share one GPU to validate the multi-rank path on a 1-GPU box)")
    ap.add_argument("--exchange-via-allreduce", action="store_true", help="several ranks: route the neighbour exchanges through all-reduces of zero-padded buffers instead of ncclSend / ncclRecv (PGO_EXCHANGE_VIA_ALLREDUCE=1: the safety net for a node where RCCL's point-to-point path misbehaves; moves world x the bytes)")
    ap.add_argument("--no-ceres-rule", action="store_true", help="skip the untimed leg that repeats the K iterations with the early-rejection pauses off (Ceres' exact decision rule)")
    ap.add_argument("--mg-dist-min-rows", type=int, default=None, help="several ranks: pgo_options.mg_dist_min_rows (library default 8192) — multigrid levels with at least this many rows are distributed; the knob to tune on a real node (DESIGN.md section 8)")
    ap.add_argument("--mg-dist-setup", type=int, default=None, choices=[0, 1], help="several ranks: pgo_options.mg_dist_setup (library default 1: the multigrid's set-up distributed like its cycle; 0: rounds 3-5's replicated set-up)")
    ap.add_argument("--partition", choices=["spatial", "chain", "contiguous"], default="spatial", help="how edges are dealt out to the ranks (solve_keyframe_pose_graph_amd/sharding.py)")
    ap.add_argument("--no-c5-strong", action="store_true", help="several ranks, default config: skip the extra BASELINE-config-5 leg (1M poses / 3M edges sharded over the ranks) that is appended as `c5_strong`")
    ap.add_argument("--c5-timeout", type=int, default=300, help="watchdog of that leg, seconds")
    ap.add_argument("--multi-timeout", type=int, default=900, help="several ranks: watchdog of the WHOLE run up to the bench line, seconds — a collective that never comes back (RCCL's point-to-point path has "
                    "never run between two physical GPUs in this repo) ends the run with an error line instead of hanging; retry with --exchange-via-allreduce")
    ap.add_argument("--config", choices=["C3", "C5"], default="C3",
                    help="C3 (default): the headline workload, N x C3 on N GPUs = WEAK scaling (what the driver's `bench.py --gpus N` runs).  C5: BASELINE.json config 5 — 1M poses / "
                         "3M edges, the SAME graph whatever N, edges sharded over the ranks = STRONG scaling; `value` is then LM iterations/s of that one graph")
    args = ap.parse_args()

    if args.exchange_via_allreduce:
        os.environ["PGO_EXCHANGE_VIA_ALLREDUCE"] = "1"      # (read by libpgo once, at its first exchange)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            raise SystemExit("--gpus %d needs torch.distributed.run with --nproc-per-node %d" % (args.gpus, args.gpus))
        args.gpus = world

    # stdout carries exactly ONE line, the JSON of rank 0.  Native libraries print on stdout behind Python's back (librccl a version
    # banner at exit, gloo its connection report), so file descriptor 1 is pointed at stderr for the whole run and the result line is
    # written to a private duplicate of the original stdout.
    result_fd = os.dup(1)
    os.dup2(2, 1)

    import torch
    dist = None
    device_index = local_rank
    if world > 1:
        import torch.distributed as dist
        if args.collective == "rccl":
            torch.cuda.set_device(local_rank)
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank))
        else:
            device_index = local_rank % max(1, torch.cuda.device_count())
            torch.cuda.set_device(device_index)
            dist.init_process_group(backend="gloo")
    elif torch.cuda.is_available():
        torch.cuda.set_device(0)
        device_index = 0

    from solve_keyframe_pose_graph_amd import capi, graphgen
    capi.load()   # raises if libpgo.so is missing: no CPU fallback

    # ---- workload: N x C3, generated identically on every rank (deterministic); edges dealt out by the `--partition` policy
    strong = args.config == "C5"
    scale = 1 if strong else args.gpus
    if strong:
        g = graphgen.config("C5")
    else:
        n_poses = args.poses_per_gpu * scale
        n_loops = int(round(C3_LOOPS * (args.poses_per_gpu / C3_POSES))) * scale if scale > 1 or args.poses_per_gpu != C3_POSES else C3_LOOPS
        g = graphgen.generate(n_poses, n_loops, odom_f_max=2, seed=3)
    n_edges = g.n_odom + g.n_loops

    from solve_keyframe_pose_graph_amd import sharding
    shard, shard_stats = None, None
    if world > 1:
        parts = sharding.partition(g, world, args.partition)
        shard = parts[rank]
        if rank == 0:
            shard_stats = sharding.partition_stats(g, parts)

    opt = {}
    if args.mg_dist_min_rows is not None:
        opt["mg_dist_min_rows"] = args.mg_dist_min_rows
    if args.mg_dist_setup is not None:
        opt["mg_dist_setup"] = args.mg_dist_setup
    if args.cg_tol is not None:
        opt["cg_rel_tolerance"] = args.cg_tol
    if args.cg_max is not None:
        opt["cg_max_iterations"] = args.cg_max
    gloo_allreduce = None
    if world > 1 and args.collective == "gloo":
        import ctypes
        hip = ctypes.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        hip.hipStreamSynchronize.argtypes = [ctypes.c_void_p]

        def gloo_allreduce(buf, count, op, stream):
            hip.hipStreamSynchronize(stream)
            host = torch.empty(count, dtype=torch.float64)
            hip.hipMemcpy(host.data_ptr(), buf, count * 8, 2)
            dist.all_reduce(host, op=dist.ReduceOp.SUM if op == 0 else dist.ReduceOp.MAX)
            hip.hipMemcpy(buf, host.data_ptr(), count * 8, 1)
            return 0

        def gloo_exchange(sbuf, soff, rbuf, roff, stream):
            """the neighbour exchange through torch.distributed point-to-point (host staging: a functional path, not a fast one)"""
            hip.hipStreamSynchronize(stream)
            send = torch.empty(max(soff[-1], 1), dtype=torch.float64)
            recv = torch.empty(max(roff[-1], 1), dtype=torch.float64)
            if soff[-1]:
                hip.hipMemcpy(send.data_ptr(), sbuf, soff[-1] * 8, 2)
            reqs = []
            for q in range(world):
                if q == rank:
                    continue
                if soff[q + 1] > soff[q]:
                    reqs.append(dist.isend(send[soff[q]:soff[q + 1]], dst=q))
                if roff[q + 1] > roff[q]:
                    reqs.append(dist.irecv(recv[roff[q]:roff[q + 1]], src=q))
            for r_ in reqs:
                r_.wait()
            if roff[-1]:
                hip.hipMemcpy(rbuf, recv.data_ptr(), roff[-1] * 8, 1)
            return 0

    def make_problem(graph=None, graph_shard=None):
        """A FRESH handle: the library keeps per-handle history between solves (which preconditioner paid last time, for the incremental
        triggers of a session), so every leg of the benchmark — warm-up, timed, including-transfers — gets its own handle and the timed
        region is a function of (graph, options) alone."""
        P = capi.problem_from_graph(graph if graph is not None else g, switchable=True, edge_slice=(graph_shard if graph is not None else shard) if world > 1 else None, device_id=device_index, max_num_iterations=10 ** 6, **opt)
        if world > 1 and args.collective == "rccl":
            uid = [capi.Problem.comm_unique_id() if rank == 0 else None]
            dist.broadcast_object_list(uid, src=0)
            P.comm_init(rank, world, uid[0])
        elif world > 1:
            P.comm_init_custom(rank, world, gloo_allreduce)
            P.comm_set_exchange(gloo_exchange)
        return P

    def drop_problem(P):
        if world > 1:
            P.comm_destroy()
        P.close()

    main_dog = None
    if world > 1 and args.multi_timeout > 0:
        import threading

        def main_give_up():
            if rank == 0:
                os.write(result_fd, (json.dumps({"metric": "LM iters/sec + final chi2 vs Ceres, 100k-pose/300k-edge SE(3) graph", "value": None, "unit": "LM iters/s", "n_gpus": args.gpus, "steps": args.steps,
                                                 "warmup": args.warmup, "error": "no result after %d s with %d ranks over '%s' (a collective did not come back?); retry with --exchange-via-allreduce" % (args.multi_timeout, world, args.collective)}) + "\n").encode())
            os._exit(3)
        main_dog = threading.Timer(args.multi_timeout, main_give_up)
        main_dog.daemon = True
        main_dog.start()
    P = make_problem()
    q0, t0_, s0 = g.init_q, g.init_t, np.full(g.n_loops, 0.99)

    def sync():
        P.synchronize()
        if torch.cuda.is_available():
            torch.cuda.synchronize()

    def barrier():
        if dist is not None:
            dist.barrier()

    # ---- warmup (untimed): W LM iterations from the initial guess, then reset the state
    P.solve_begin(q0, t0_, s0)
    for _ in range(args.warmup):
        P.lm_step(ignore_termination=True)
    P.solve_end()
    fresh = world == 1     # several ranks: ONE handle and ONE communicator for all legs (the multi-rank PCG keeps no history between solves)
    if fresh:
        drop_problem(P)

    # ---- timed: exactly K LM iterations from the odometry initial guess, state resident in HBM (fresh handle; upload, device graph build and
    # iteration 0 happen in solve_begin, outside the timed region)
    if fresh:
        P = make_problem()
    P.solve_begin(q0, t0_, s0)
    barrier(); sync()
    t_start = time.perf_counter()
    for _ in range(args.steps):
        P.lm_step(ignore_termination=True)
    sync(); barrier()
    elapsed = time.perf_counter() - t_start
    if dist is not None:
        tt = torch.tensor([elapsed], dtype=torch.float64, device="cuda" if args.collective == "rccl" else "cpu")
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())

    shard_counters = P.sharding_stats().as_dict() if world > 1 else None
    cg_ms = cg_bytes = mv_ms = mv_bytes = up_ms = up_bytes = None
    mg_ms = mg_bytes = mgc_ms = mgc_bytes = None
    if args.full:      # (pgo_time_kernel leaves the keyframe state of the open solve as it is: what solve_end returns below is the timed steps' result)
        # ---- roofline of the dominant data-parallel kernel (K1), measured live with HIP events on the library stream
        k1_ms, k1_bytes = P.time_kernel(0, 50)
        k2_ms, k2_bytes = P.time_kernel(1, 20)
        if world == 1:
            cg_ms, cg_bytes = P.time_kernel(2, 50)
            mv_ms, mv_bytes = P.time_kernel(4, 50)
            try:
                up_ms, up_bytes = P.time_kernel(5, 50)
            except capi.PgoError:      # single-reduction form: the update cannot run without its matvec (its head would see stale partial sums): iteration minus matvec
                up_ms, up_bytes = cg_ms - mv_ms, cg_bytes - mv_bytes
        # (several ranks: the single-GPU form of the PCG iteration is not what they run: no such figure for them)
        k1c_ms, k1c_bytes = P.time_kernel(3, 50)
        try:      # one multigrid-preconditioned PCG iteration on the current LM system (graphs with a hierarchy: >= mg_min_keyframes keyframes, one GPU)
            if world == 1:
                mg_ms, mg_bytes = P.time_kernel(6, 50)
                mgc_ms, mgc_bytes = P.time_kernel(7, 50)
        except capi.PgoError:
            pass
    qf, tf, sf, summ = P.solve_end()
    P_linear_solver, P_cg_tol, P_cg_max = P.options.linear_solver, P.options.cg_rel_tolerance, P.options.cg_max_iterations
    summ_cg_total = int(summ.cg_iterations)
    summ_cg_mg = int(summ.cg_iterations_multigrid)
    if fresh:
        drop_problem(P)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, qf, tf, sf, summ)

    # ---- the same K iterations once more INCLUDING the host<->device transfers and the write-back; never `value`
    elapsed_incl = None
    if args.full:
        if fresh:
            P = make_problem()   # cold handle: the edge upload and the device graph build of a first solve are part of this figure
        barrier(); sync()
        t_incl = time.perf_counter()
        P.solve_begin(q0, t0_, s0)
        for _ in range(args.steps):
            P.lm_step(ignore_termination=True)
        P.solve_end()
        sync(); barrier()
        elapsed_incl = time.perf_counter() - t_incl
    if args.full or not fresh:
        drop_problem(P)

    # ---- K1 once more where its output cannot sit in the 256 MiB Infinity Cache: C3's 194 MB of Jacobian blocks are absorbed by it (plain
    # stores), so the C3 figure is an HBM + cache number; 400k keyframes / 1.2M edges write 775 MB with non-temporal stores
    k1_big = None
    if args.full and scale == 1 and world == 1 and not strong and rank == 0 and not args.no_k1_out_of_cache:
        gb = graphgen.generate(400000, 400000, odom_f_max=2, seed=3)
        Pb = capi.problem_from_graph(gb, switchable=True, device_id=device_index)
        Pb.solve_begin(gb.init_q, gb.init_t, np.full(gb.n_loops, 0.99))
        ms_b, by_b = Pb.time_kernel(0, 30)
        Pb.solve_end(); Pb.close()
        k1_big = {"workload": "400000 poses / %d edges, same generator" % (gb.n_odom + gb.n_loops), "achieved": by_b / (ms_b * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                  "frac": by_b / (ms_b * 1e-3) / 1e9 / HBM_PEAK_GBS, "algorithmic_bytes_per_launch": by_b, "avg_launch_ms": ms_b}
        del gb

    # ---- the same K iterations under Ceres' EXACT decision rule: cg_early_tolerance = cg_mid_tolerance = 0 — every step's linear system is solved to
    # cg_rel_tolerance before it is accepted or rejected, as an exact factorisation would.  Outside the timed `value`; reported beside it.
    ceres_rule = None
    if args.full and scale == 1 and world == 1 and not strong and not args.no_ceres_rule:
        try:
            Pe = capi.problem_from_graph(g, switchable=True, device_id=device_index, max_num_iterations=10 ** 6, cg_early_tolerance=0.0, cg_mid_tolerance=0.0, **opt)
            Pe.solve_begin(q0, t0_, s0)
            Pe.synchronize()
            te0 = time.perf_counter()
            for _ in range(args.steps):
                Pe.lm_step(ignore_termination=True)
            Pe.synchronize()
            te = time.perf_counter() - te0
            _, _, _, sume = Pe.solve_end()
            Pe.close()
            ite = [sume.iterations[k] for k in range(sume.num_logged)]
            ceres_rule = {"value": args.steps / te, "unit": "LM iters/s", "seconds": te, "chi2_final": 2.0 * sume.final_cost, "cg_iterations_total": int(sume.cg_iterations),
                          "decisions": [int(it.step_is_successful) for it in ite[1:args.steps + 1]],
                          "decisions_equal_to_the_timed_run": [int(it.step_is_successful) for it in ite[1:args.steps + 1]] == [int(summ.iterations[k].step_is_successful) for k in range(1, min(summ.num_logged, args.steps + 1))],
                          "note": "both early-rejection pauses off: a rejected step pays its full linear solve, as under an exact factorisation"}
        except Exception as e:
            ceres_rule = {"error": repr(e)}

    # ---- final chi^2 against the independent CPU trajectory of the same K iterations (tests/golden/make_c3_trajectory.py: oracle Jacobians,
    # scipy CG to 1e-12, Python restatement of the Ceres LM loop; nothing of libpgo)
    chi2_ref = chi2_rel = None
    if scale == 1 and world == 1 and not strong and args.poses_per_gpu == C3_POSES:
        for name in ("c3_twenty_iterations.json", "c3_ten_iterations.json"):
            try:
                with open(os.path.join(ROOT, "tests", "golden", name)) as f:
                    gold = json.load(f)["iterations"]
                if args.steps < len(gold):
                    chi2_ref = 2.0 * gold[args.steps]["cost"]
                    chi2_rel = abs(2.0 * summ.final_cost - chi2_ref) / chi2_ref
                    break
            except Exception:
                pass

    # ---- parity at the CONVERGED minimum (BASELINE.json "final chi^2 within 1e-6 relative"): the same graph solved once more, outside every timed
    # region, with the reference's options left at Ceres' defaults (function_tolerance 1e-6) until the minimiser stops by itself, against the independent CPU run to
    # convergence (tests/golden/c3_converged.json: oracle Jacobians + scipy CG to 1e-12 + Python restatement of the Ceres loop; nothing of libpgo)
    chi2_conv = None
    if args.full and scale == 1 and world == 1 and not strong and args.poses_per_gpu == C3_POSES:
        try:
            with open(os.path.join(ROOT, "tests", "golden", "c3_converged.json")) as f:
                gold = json.load(f)
            Pc = capi.problem_from_graph(g, switchable=True, device_id=device_index, max_num_iterations=int(gold.get("max_iterations", 400)), **opt)
            tc0 = time.perf_counter()
            qc, tc, sc, sumc = Pc.solve(q0, t0_, s0)
            tc1 = time.perf_counter()
            Pc.close()
            ref = np.array(gold["final_t_sample_100"])
            on_ref = np.unpackbits(np.frombuffer(bytes.fromhex(gold["switches_on_hex"]), dtype=np.uint8))[:gold["n_switches"]]
            chi2_conv = {"chi2_converged": 2.0 * sumc.final_cost, "chi2_converged_ref": gold["final_chi2"], "chi2_converged_rel_diff": abs(2.0 * sumc.final_cost - gold["final_chi2"]) / gold["final_chi2"],
                         "lm_iterations": int(sumc.num_iterations), "lm_iterations_ref": len(gold["iterations"]) - 1, "termination": sumc.message.decode(), "termination_ref": gold.get("termination"),
                         "seconds": tc1 - tc0, "max_position_diff_m_every_100th_keyframe": float(np.abs(tc.reshape(-1, 3)[::100] - ref).max()),
                         "switches_on_opposite_side_of_0.5": int(np.count_nonzero((sc > 0.5).astype(np.uint8) != on_ref))}
        except FileNotFoundError:
            chi2_conv = None
        except Exception as e:
            chi2_conv = {"error": repr(e)}

    # Static PMC traffic figures (rocprofv3 --pmc passes cannot run inside this process: scripts/profile_r03_final.sh -> profiles/*_pmc_latest.json) are reported only
    # when they were measured on THIS build: every file carries the sha256 of the libpgo.so it profiled.
    import hashlib
    from solve_keyframe_pose_graph_amd import _build as _b
    with open(os.environ.get("PGO_LIBPGO_OVERRIDE") or _b.LIBPGO, "rb") as f:
        lib_sha = hashlib.sha256(f.read()).hexdigest()
    traffic_note = {}

    def static_traffic(name, getter):
        if not (args.full and scale == 1 and world == 1 and not strong and args.poses_per_gpu == C3_POSES):
            return None        # the PMC passes were taken on C3 x 1 only (and stand beside the rooflines of --full)
        try:
            with open(os.path.join(ROOT, "profiles", name)) as f:
                pj = json.load(f)
            if pj.get("libpgo_sha256") != lib_sha:
                traffic_note[name] = "refused: profiled on libpgo.so %s, this run loaded %s" % (str(pj.get("libpgo_sha256"))[:12], lib_sha[:12])
                return None
            return getter(pj)
        except Exception as e:
            traffic_note[name] = "unavailable: %r" % (e,)
            return None
    traffic = static_traffic("k1_pmc_latest.json", lambda pj: pj["hbm_bytes_per_launch"])
    pcg_traffic = static_traffic("pcg_pmc_latest.json", lambda pj: pj["matvec"]["hbm_bytes_per_launch"] + pj["update"]["hbm_bytes_per_launch"])
    mg_traffic = static_traffic("mg_pmc_latest.json", lambda pj: pj["hbm_bytes_per_iteration"])
    # ---- several ranks, default (weak) run: BASELINE.json config 5 as well — the SAME 1M-pose / 3M-edge graph whatever N, its edges sharded over the ranks (strong scaling) —
    # so that a scaling run carries the configured multi-GPU workload next to the weak N x C3 `value`.  A bounded leg: at most 5 LM iterations after 1 warm-up iteration.
    def run_c5_strong():
        try:
            g5 = graphgen.config("C5")
            parts5 = sharding.partition(g5, world, args.partition)
            stats5 = sharding.partition_stats(g5, parts5) if rank == 0 else None
            k5 = max(1, min(args.steps, 5))
            P5 = make_problem(g5, parts5[rank])
            q5, t5, s5 = g5.init_q, g5.init_t, np.full(g5.n_loops, 0.99)
            P5.solve_begin(q5, t5, s5)
            P5.lm_step(ignore_termination=True)
            P5.solve_end()
            P5.solve_begin(q5, t5, s5)
            barrier(); P5.synchronize()
            t5_0 = time.perf_counter()
            for _ in range(k5):
                P5.lm_step(ignore_termination=True)
            P5.synchronize(); barrier()
            el5 = time.perf_counter() - t5_0
            tt = torch.tensor([el5], dtype=torch.float64, device="cuda" if args.collective == "rccl" else "cpu")
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            el5 = float(tt.item())
            counters5 = P5.sharding_stats().as_dict()
            _, _, _, sum5 = P5.solve_end()
            drop_problem(P5)
            if rank == 0:
                return {"workload": "C5: synthetic 3D Manhattan graph, %d poses / %d edges, the same graph on every rank count (BASELINE.json config 5), edges sharded by the '%s' policy" % (g5.n_poses, g5.n_odom + g5.n_loops, args.partition),
                             "scaling": "strong", "steps": k5, "seconds": el5, "lm_iters_per_s": k5 / el5, "chi2_final": 2.0 * sum5.final_cost, "cg_iterations_total": int(sum5.cg_iterations),
                             "cg_iterations_multigrid": int(sum5.cg_iterations_multigrid), "shared_keyframes": stats5["shared_keyframes"], "edges_per_rank": [min(stats5["edges_per_rank"]), max(stats5["edges_per_rank"])],
                             "sharding_counters": counters5,
                             "note": "per CG iteration: neighbour exchange of the shared keyframes' rows + one 2-double all-reduce; multigrid cycle distributed (levels >= mg_dist_min_rows rows run on their owners' rows, halo rows by neighbour exchange, smaller levels by every rank from gathered vectors); the multigrid's SET-UP distributed the same way (every rank forms the operators of its own rows, shared blocks by neighbour exchange, the first completely-run level gathered, the dense inverse on every rank: DESIGN.md §8)"}
            return None
        except Exception as e:      # the weak figure above is the contract; this leg is reported when it runs
            return {"error": repr(e)}

    if main_dog is not None:
        main_dog.cancel()      # (everything the contract asks for has been measured; the C5 leg below has a watchdog of its own)
    out = None
    written = [False]
    if rank == 0:
        ips = args.steps / elapsed
        its = [summ.iterations[k] for k in range(summ.num_logged)]
        out = {
            "metric": "LM iters/sec + final chi2 vs Ceres, 100k-pose/300k-edge SE(3) graph" if not strong else "LM iters/sec, 1M-pose/3M-edge SE(3) graph (BASELINE.json config 5) edge-sharded over the ranks",
            "value": ips * scale,
            "unit": "LM iters/s" if scale == 1 else "LM iters/s x N (C3-sized graph-iterations/s)",
            "n_gpus": args.gpus, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": 1e3 * elapsed / args.steps,
            "higher_is_better": True, "scaling": "strong" if strong else "weak", "vs_baseline": None,
            "dtype": "f64", "data": "synthetic",
            "config": {"workload": "%s: synthetic 3D Manhattan graph, %d poses / %d edges (%d odometry f=1,2 + %d switchable loop closures, 10%% outliers) + %d regulariser(s)"
                                   % ("C5 (the same graph on every rank count)" if strong else "C3 x %d" % scale, g.n_poses, n_edges, g.n_odom, g.n_loops, len(g.reg_node)),
                       "poses": g.n_poses, "edges": n_edges, "sharding": ("edges by the '%s' policy (sharding.py): %d..%d edges and %d..%d keyframes per rank, %d of %d keyframes shared between ranks; per CG iteration the partial rows of the matvec output go to the ranks sharing a keyframe (neighbour send / receive, summed in rank order) + one %s all-reduce of 2 doubles; the multigrid's cycle AND set-up are distributed (every rank runs the level kernels and forms the level operators on the rows it owns; halo rows, and the blocks two ranks share, by neighbour exchange: sharding_counters)"
                                                                       % (args.partition, min(shard_stats["edges_per_rank"]), max(shard_stats["edges_per_rank"]), min(shard_stats["keyframes_per_rank"]), max(shard_stats["keyframes_per_rank"]),
                                                                          shard_stats["shared_keyframes"], g.n_poses, args.collective)) if world > 1 else "single GPU",
                       "linear_solver": "PCG on the Schur-reduced pose system, %s matvec; 6x6 block-Jacobi, hard LM systems by the aggregation multigrid (hybrid start)" % ("matrix-free" if P_linear_solver == 1 else "block-CSR"), "cg_rel_tolerance": P_cg_tol,
                       "cg_max_iterations": P_cg_max, "library_options_set_on_the_command_line": opt or None},
            # several ranks: what THIS rank's exchanges moved and what its level kernels work on (pgo_get_sharding_stats, rank 0's view; bytes_round5_*: what round 5's union
            # all-reduce carried on the same graph).  Nothing multi-GPU in this repo has been timed on hardware before this run.
            "sharding_counters": shard_counters,
            # (several ranks) what the weak leg's graph costs on ONE GPU as it grows — measured in round 6 (profiles/r06_weak_graph_growth.txt), quoted here so that an efficiency computed
            # from the values of N = 1, 2, 4, 8 is read with the problem's own growth beside it
            "weak_graph_note": ("N x C3 as ONE graph is a harder problem at every N: 10 LM iterations on one MI355X take 0.092 / 0.43 / 0.98 / 2.25 / 10.7 s at N = 1 / 2 / 4 / 6 / 8 "
                                "(every step of the 800 000-keyframe graph is accepted, the trust region opens to 2.4e7, 20 441 PCG iterations instead of 798); the c5_strong leg — the same "
                                "graph at every N — isolates the solver's scaling") if world > 1 and not strong else None,
            "libpgo_sha256": lib_sha,
            # the hash of the sources the loaded library was built from (compiled in by _build.py) next to the hash of this checkout's sources: equal = built from this tree
            "libpgo_sources_sha256": capi.build_info()[0], "checkout_sources_sha256": capi.build_info()[1],
            "lm_iters_per_s_raw": ips,
            "chi2_initial": 2.0 * summ.initial_cost, "chi2_final": 2.0 * summ.final_cost,
            "chi2_ref": chi2_ref, "chi2_rel_diff": chi2_rel,   # reference = the CPU trajectory after the same number of LM iterations (null: no golden for this workload / step count)
            "lm_successful_steps": summ.num_successful_steps, "cg_iterations_total": int(summ.cg_iterations),
            "cg_iterations_per_step": [it.cg_iterations for it in its[1:]],
            # what the K counted LM iterations were: a step rejected at an early-rejection pause costs a fraction of a fully solved one (Ceres pays a full factorisation for each)
            "lm_iterations_fully_solved": sum(1 for it in its[1:] if it.reason != capi.STEP_REJECTED_AT_PAUSE),
            "lm_iterations_rejected_at_pause": sum(1 for it in its[1:] if it.reason == capi.STEP_REJECTED_AT_PAUSE),
            "pcg_form": "single-reduction (Chronopoulos-Gear)" if any(it.single_reduction for it in its[1:]) else "classic (two reductions per iteration)",
            # where the timed region went, from the library's own host clock around its device-synchronised phases (pgo_iteration.seconds_*)
            "timed_region_breakdown": (lambda steps: {
                "system_and_preconditioner_setup_s": sum(it.seconds_system for it in steps),
                "pcg_s_steps_ending_under_the_multigrid": sum(it.seconds_pcg for it in steps if (it.preconditioner & 15) == capi.PRECOND_MULTIGRID),
                "pcg_s_other_steps": sum(it.seconds_pcg for it in steps if (it.preconditioner & 15) != capi.PRECOND_MULTIGRID),
                "candidate_evaluation_s": sum(it.seconds_evaluate for it in steps),
                "linearisation_s": sum(it.seconds_linearize for it in steps),
                "unaccounted_s": elapsed - sum(it.seconds for it in steps),
                "pcg_s_beyond_iterations_x_iteration_time": None if cg_ms is None or mg_ms is None else
                    sum(it.seconds_pcg for it in steps) - 1e-3 * (summ_cg_mg * mg_ms + (summ_cg_total - summ_cg_mg) * cg_ms),
                "note": "pcg_s includes the early-rejection pauses' candidate evaluations, the drain of the chunk in flight when a PCG stops, and multigrid operators built after a PCG has started (in-flight switch)"})(its[1:args.steps + 1]),
        }
    if rank == 0 and args.full:
        out.update({
            "static_traffic_notes": traffic_note or None, "c5_strong": None,
            "value_ceres_decision_rule": ceres_rule,
            "lm_iters_per_s_including_transfers": args.steps / elapsed_incl * scale,   # upload of the state, K iterations, write-back (rank 0's clock)
            "chi2_converged_rel_diff": None if not chi2_conv or "error" in chi2_conv else chi2_conv["chi2_converged_rel_diff"], "converged": chi2_conv,
            "roofline": {"bound": "hbm", "kernel": "k1_edges_kernel<true> (residual + Jacobian blocks, all edges, one launch)",
                         "achieved": k1_bytes / (k1_ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": k1_bytes / (k1_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, "traffic": traffic,
                         "traffic_source": "static: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this kernel on C3 (profiles/k1_pmc_latest.json), not measured in this run",
                         "algorithmic_bytes_per_launch": k1_bytes, "avg_launch_ms": k1_ms,
                         "note": "frac is the C3 figure (the benchmark workload); its 194 MB output fits the 256 MiB Infinity Cache — roofline_k1_out_of_cache is the HBM-only figure"},
            "roofline_k1_out_of_cache": k1_big,
            # where the solve spends its time: one block-Jacobi PCG iteration = matvec + vector update, bytes = what this design moves per iteration
            "roofline_pcg": None if cg_ms is None else {"bound": "hbm", "kernel": "%s + cg_update_kernel (one PCG iteration)" % ("mf_spmv_kernel<true>" if P_linear_solver == 1 else "cg_spmv_kernel"),
                             "achieved": cg_bytes / (cg_ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": cg_bytes / (cg_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                             "algorithmic_bytes_per_iteration": cg_bytes, "avg_iteration_ms": cg_ms, "traffic": pcg_traffic,
                             "traffic_source": "static: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of the two kernels on C3 (profiles/pcg_pmc_latest.json), not measured in this run",
                             "matvec": {"ms": mv_ms, "bytes": mv_bytes, "GBps": mv_bytes / mv_ms / 1e6}, "update": {"ms": up_ms, "bytes": up_bytes, "GBps": up_bytes / up_ms / 1e6},
                             "iterations_in_timed_region": summ_cg_total - summ_cg_mg,
                             "share_of_timed_region": (summ_cg_total - summ_cg_mg) * cg_ms * 1e-3 / elapsed},
            # the hard LM systems run the same PCG preconditioned by the aggregation multigrid: matvec + update with the restriction + the level kernels
            "roofline_mg": None if mg_ms is None else {
                "bound": "hbm", "kernel": "mf_spmv_kernel<true> + cg_update_mg_kernel + mg_down / mg_dense_solve / mg_up kernels (one multigrid-preconditioned PCG iteration)",
                "achieved": mg_bytes / (mg_ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": mg_bytes / (mg_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                "algorithmic_bytes_per_iteration": mg_bytes, "avg_iteration_ms": mg_ms, "traffic": mg_traffic,
                "traffic_source": "static: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of every kernel of the iteration on C3 (profiles/mg_pmc_latest.json, same libpgo.so sha256), not measured in this run",
                "cycle_kernels": {"ms": mgc_ms, "bytes": mgc_bytes, "GBps": mgc_bytes / mgc_ms / 1e6},
                "iterations_in_timed_region": summ_cg_mg, "share_of_timed_region": summ_cg_mg * mg_ms * 1e-3 / elapsed,
                "note": "latency-bound: the coarse levels hold 12 %, 4 %, 1 % and 0.4 % of the keyframes, every level kernel starts on cold L2s (DESIGN.md)"},
            "other_kernels": {"k2_assembly": {"ms": k2_ms, "GBps": k2_bytes / k2_ms / 1e6}, "pcg_iteration": None if cg_ms is None else {"ms": cg_ms, "GBps": cg_bytes / cg_ms / 1e6},
                              "k1_cost_only": {"ms": k1c_ms, "GBps": k1c_bytes / k1c_ms / 1e6}},
        })
        if scale == 1 and world == 1 and not strong and not args.no_cpu_baseline:
            try:
                out["cpu_baseline"] = cpu_baseline(args.cpu_sample_poses, args.cpu_iters, 30.0)
            except Exception as e:   # the baseline is reported, never required for the GPU number
                out["cpu_baseline"] = {"value": None, "unit": "LM iters/s (C3-equivalent)", "cores": 1, "kind": "port", "sample": "failed: %r" % (e,)}
    if args.full and world > 1 and not strong and not args.no_c5_strong:
        # The C5 leg runs LAST, after everything the contract asks for has been measured, under a watchdog on every rank: a collective that does not come back on some
        # multi-GPU box must cost this leg, not the bench line — after --c5-timeout seconds rank 0 prints the line without it and every rank leaves.
        import threading
        write_lock = threading.Lock()

        def give_up():
            with write_lock:      # (the main path takes the same lock around ITS write: exactly one line is ever written)
                if written[0]:
                    return
                if rank == 0:
                    out["c5_strong"] = {"error": "timed out after %d s (the weak-scaling figures above are complete)" % args.c5_timeout}
                    os.write(result_fd, (json.dumps(out) + "\n").encode())
                written[0] = True
                os._exit(0)
        dog = threading.Timer(args.c5_timeout, give_up)
        dog.daemon = True
        dog.start()
        c5 = run_c5_strong()
        dog.cancel()
        with write_lock:
            if rank == 0:
                out["c5_strong"] = c5
                os.write(result_fd, (json.dumps(out) + "\n").encode())
            written[0] = True
    elif rank == 0:
        os.write(result_fd, (json.dumps(out) + "\n").encode())
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
