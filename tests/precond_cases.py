"""What tests/test_precond_model.py (CPU) and tests/test_gpu_precond_operator.py (GPU) share: the graphs, their linearisations by the CPU checker (computed once
per process), the constant-keyframe sets, and — CPU only — the multigrid aggregates from the host shim (tests/native/mg_host.cpp) built with the arguments
pgo_multigrid.hip hands build_hierarchy on one GPU.

The multigrid graph's seed was picked on the CPU: the smoother-limit estimate omega * lambda (launch_mg_level_power, emulated by precond_model.power_estimate) of
every sparse level of every hierarchy used here is 1.68 - 1.72 at both radii, in fp64 and with the fp32 level matrices, i.e. clear of the limit 1.75 the rescaling
starts at (seeds 3, 7 and 11 sit at 1.72 - 1.755: the decision would then hang on the last digits of the estimate).

mgyaw640 is the graph on which the rescaling DOES start, on one sparse level and not on the other (MG_PATH_CASES): f = 1..5 with yaw weights and turns of 3 degrees per
keyframe, the hierarchy of mg_passes = 2, mg_dense_max_nodes = 16 (levels 114 / 37 / 12).  Its seed was picked the same way, among 3, 5, 7 and 11, omega * lambda of
(level 1, level 2) at the two radii, the same in fp64 and with the fp32 level matrices:
  seed  plain transitions            one smoothed transition      smoothed keyframe transition + one smoothed transition
  3     1.698, 1.766 / 1.698, 1.767  1.698, 1.977 / 1.698, 1.974  1.710, 1.7475 / 1.712, 1.791   (level 2 of the last within 0.003 of the limit)
  5     1.731, 1.804 / 1.733, 1.805  1.731, 1.815 / 1.733, 1.824  2.146, 1.685 / 2.154, 1.713
  7     1.7445, 1.772 / 1.746, 1.777 1.7445, 1.703 / 1.746, 1.740 1.766, 1.607 / 1.771, 1.674    (level 1 within 0.006)
  11    1.775, 1.766 / 1.776, 1.764  1.775, 2.269 / 1.776, 2.234  1.805, 1.644 / 1.810, 1.693    (both levels above the limit in the first two: nothing tells them apart)
Seed 5 is the one whose every level keeps 0.017 or more from 1.75 in all three hierarchies, with one level on each side.  The regroup cases (MG_REGROUP_CASES) stay on mg640:
with its 13 outlier loop closures at s = 0.02 the rebuilt hierarchy moves 4 + 1 parents of the two sparse levels and renumbers level 1, and every estimate stays 0.03 or more
below the limit.  The GPU tests assert the same margins on the hierarchy the DEVICE installs; should one land inside, another seed or hierarchy shape is to be scanned here, not
the margin loosened."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

from solve_keyframe_pose_graph_amd import capi
from tests import precond_model as pm
from tests import util

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

RADII = (1e4, 1e7)      # the second: the largest of the decades 1e4 .. 1e7 the solver's radius rule reaches on these graphs; the model's fp32 Ac^-1 is positive definite at all of them (test_precond_model.py)
PERTURB, STATE_SEED = 0.02, 6
REGROUP_S = 0.02        # state B of the regroup cases: the switch of every outlier loop closure

# name -> (keyframes, loops, f, seed[, generator keywords])
GRAPHS = {
    "bj300": (300, 40, 4, 11),
    "tl200": (200, 25, 2, 11),
    "tl600": (600, 75, 3, 11),
    "tl601": (601, 75, 3, 11),
    "mg640": (640, 80, 5, 5),
    "mgyaw640": (640, 80, 5, 5, dict(apply_yaw_weight=1, turn_deg_per_keyframe=3.0)),      # f = 1..5 with yaw weights on gentle turns: the smoother's safety rescaling triggers
}
# constant keyframes: a whole aggregate of ten (20-29), half of another (45-49) and — unreferenced, see graph() — the last three keyframes of the two-level graph; a run in mid-trajectory
# of the multigrid graph
CONSTANT_TL600 = tuple(range(20, 30)) + tuple(range(45, 50))
CONSTANT_MG640 = tuple(range(300, 330))


@functools.lru_cache(maxsize=None)
def graph(name, drop_last=0):
    """drop_last: the last `drop_last` keyframes lose every edge (unreferenced keyframes at the end of the trajectory)"""
    n, loops, f, seed, *kw = GRAPHS[name]
    g = util.small_graph(n, loops, f=f, seed=seed, **(kw[0] if kw else {}))
    if drop_last:
        lim = n - drop_last
        ko = (g.odom_c1 < lim) & (g.odom_c2 < lim)
        kl = (g.loop_c1 < lim) & (g.loop_c2 < lim)
        kr = g.reg_node < lim
        g.odom_c1, g.odom_c2, g.odom_T, g.odom_w = g.odom_c1[ko], g.odom_c2[ko], g.odom_T[ko], g.odom_w[ko]
        g.loop_c1, g.loop_c2, g.loop_T, g.loop_w, g.loop_is_outlier = g.loop_c1[kl], g.loop_c2[kl], g.loop_T[kl], g.loop_w[kl], g.loop_is_outlier[kl]
        g.reg_node, g.reg_T, g.reg_w = g.reg_node[kr], g.reg_T[kr], g.reg_w[kr]
    return g


def state(g, regroup=None):
    """regroup "A": the state itself; "B": its outlier loop closures switched off (s = 0.02), poses unchanged — the start values of a second solve on the same handle"""
    q, t, s = util.initial_state(g, True, perturb=PERTURB, seed=STATE_SEED)
    if regroup == "B":
        s = s.copy()
        s[np.asarray(g.loop_is_outlier, dtype=bool)] = REGROUP_S
    return q, t, s


@functools.lru_cache(maxsize=None)
def linearisation(name, constant=(), drop_last=0, regroup=None):
    g = graph(name, drop_last)
    q, t, s = state(g, regroup)
    return pm.Linearisation(util.oracle_problem(g, True), g, q, t, s, constant)


@functools.lru_cache(maxsize=None)
def system(name, radius, constant=(), drop_last=0, regroup=None):
    return linearisation(name, constant, drop_last, regroup).system(radius)


# ---- CPU only: the aggregates of the host hierarchy builder ----
def _shim():
    so = os.path.join(HERE, "native", "libmg_host.so")
    src = os.path.join(HERE, "native", "mg_host.cpp")
    hdr = os.path.join(ROOT, "solve_keyframe_pose_graph_amd", "csrc", "pgo_mg_host.hpp")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", os.path.dirname(hdr), "-o", so, src])
    lib = C.CDLL(so)
    lib.mgh_build_regroup.restype = C.c_void_p
    lib.mgh_build_fine_sw.restype = C.c_void_p
    return lib


def host_hierarchy(g, free, s, passes, dense_max, smoothed_levels, fine=False, s_first=None):
    """(agg0 [N], parents per sparse level, level sizes) as pgo_multigrid.hip builds them on one GPU: three first passes, level-1 aggregates inside runs of 64 keyframes,
    loop discount 3, switch weights s^2.  fine: the route of the smoothed keyframe transition (mgh_build_fine: the keyframe level's block pattern handed to build_hierarchy).
    s_first: the REGROUPED hierarchy — a first build with the switches s_first fills the cache, the result is the rebuild with s from that cache (mgh_build_regroup, use_cache = 1)"""
    lib = _shim()
    I32 = lambda x: np.ascontiguousarray(x, dtype=np.int32)
    ptr = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    N = g.n_poses
    nf = np.ascontiguousarray(free, dtype=np.uint8)
    rc1, rc2, sc1, sc2 = I32(g.odom_c1), I32(g.odom_c2), I32(g.loop_c1), I32(g.loop_c2)
    rw = np.ascontiguousarray(g.odom_w, dtype=np.float64)
    sw = np.ascontiguousarray(np.asarray(s, dtype=np.float64) ** 2)
    graph_args = (C.c_longlong(N), ptr(nf, C.c_ubyte), C.c_longlong(len(rc1)), ptr(rc1, C.c_int), ptr(rc2, C.c_int), ptr(rw, C.c_double), C.c_longlong(len(sc1)), ptr(sc1, C.c_int), ptr(sc2, C.c_int))
    if fine:
        assert s_first is None
        h = lib.mgh_build_fine_sw(*graph_args, ptr(sw, C.c_double), 3, passes, dense_max, 32, 12, smoothed_levels, C.c_double(3.0), 64)
    else:
        sw0 = sw if s_first is None else np.ascontiguousarray(np.asarray(s_first, dtype=np.float64) ** 2)
        h = lib.mgh_build_regroup(*graph_args, ptr(sw0, C.c_double), ptr(sw, C.c_double), 0 if s_first is None else 1, 3, passes, dense_max, 32, 12, smoothed_levels, C.c_double(3.0), 64)
    assert h, "the graph does not coarsen"
    h = C.c_void_p(h)
    parents, sizes = [], []
    nl = lib.mgh_levels(h)
    for l in range(nl):
        sz = np.zeros(6, np.int64)
        lib.mgh_sizes(h, l, ptr(sz, C.c_longlong))
        n, nnzb, nent, npar, nagg, ntile = [int(x) for x in sz]
        rowptr, col, g_ptr, g_ent = np.zeros(n + 1, np.int64), np.zeros(nnzb, np.int32), np.zeros(nnzb + 1, np.int64), np.zeros(nent, np.int64)
        parent, agg_ptr, tile_agg0 = np.zeros(npar, np.int32), np.zeros(nagg, np.int32), np.zeros(ntile, np.int32)
        lib.mgh_level(h, l, ptr(rowptr, C.c_longlong), ptr(col, C.c_int), ptr(g_ptr, C.c_longlong), ptr(g_ent, C.c_longlong), ptr(parent, C.c_int), ptr(agg_ptr, C.c_int), ptr(tile_agg0, C.c_int))
        sizes.append(n)
        if l + 1 < nl:
            parents.append(parent)
    agg0 = np.zeros(N, np.int32)
    mem0_ptr = np.zeros(sizes[0] + 1, np.int32)
    mem0 = np.zeros(int((nf != 0).sum()), np.int32)
    lib.mgh_level0(h, ptr(agg0, C.c_int), ptr(mem0_ptr, C.c_int), ptr(mem0, C.c_int))
    lib.mgh_free(h)
    return agg0, parents, sizes


# the multigrid cases: name -> (solver options that shape the hierarchy, model arguments)
MG_CASES = {
    "dense":         (dict(mg_smoothed_levels=0, mg_dense_max_nodes=512), dict(passes=3, dense_max=512, smoothed_levels=0, explicit=False), 1),
    "one_sparse":    (dict(mg_smoothed_levels=0, mg_dense_max_nodes=64), dict(passes=3, dense_max=64, smoothed_levels=0, explicit=False), 2),
    "three_levels":  (dict(mg_smoothed_levels=0, mg_dense_max_nodes=16, mg_passes=2), dict(passes=2, dense_max=16, smoothed_levels=0, explicit=False), 3),
    "smoothed_impl": (dict(mg_smoothed_levels=1, mg_dense_max_nodes=64, mg_explicit_transfer=0), dict(passes=2, dense_max=64, smoothed_levels=1, explicit=False), 2),
    "smoothed_expl": (dict(mg_smoothed_levels=1, mg_dense_max_nodes=64, mg_explicit_transfer=1), dict(passes=2, dense_max=64, smoothed_levels=1, explicit=True), 2),
}
MG_BASE = dict(mg_min_keyframes=1, mg_min_keyframes_switchable=1, mg_smoothed_fine=0, mg_switch_iterations=0)

# the paths the library takes by default on real graphs — the smoother's safety rescaling, the smoothed keyframe transition:
# name -> (graph, solver options, model arguments, levels, per sparse level: the smoother-limit estimate rescales it)
_Y = dict(mg_dense_max_nodes=16, mg_passes=2)
_YM = dict(passes=2, dense_max=16)
MG_PATH_CASES = {
    "rescaled_plain":         ("mgyaw640", dict(_Y, mg_smoothed_levels=0), dict(_YM, smoothed_levels=0, explicit=False), 3, (False, True)),
    "rescaled_smoothed_impl": ("mgyaw640", dict(_Y, mg_smoothed_levels=1, mg_explicit_transfer=0), dict(_YM, smoothed_levels=1, explicit=False), 3, (False, True)),
    "rescaled_smoothed_expl": ("mgyaw640", dict(_Y, mg_smoothed_levels=1, mg_explicit_transfer=1), dict(_YM, smoothed_levels=1, explicit=True), 3, (False, True)),
    "fine640":                ("mg640", dict(mg_smoothed_fine=1, mg_smoothed_levels=1, mg_dense_max_nodes=64), dict(passes=2, dense_max=64, smoothed_levels=1, explicit=True, smoothed_fine=True), 2, (False,)),
    # level 1 = Ps_0^T A Ps_0 is the level that is rescaled, and the smoothed transition above it is formed with the rescaled Dinv
    "fine_rescaled":          ("mgyaw640", dict(_Y, mg_smoothed_fine=1, mg_smoothed_levels=1), dict(_YM, smoothed_levels=1, explicit=True, smoothed_fine=True), 3, (True, False)),
}
# a hierarchy after a regroup, on mg640: one handle opens a solve at state A (state(g)), closes it and opens the next at state B (state(g, "B")) — regroup_if_moved "for the
# new start" rebuilds the hierarchy from the cache; smoothed_expl: the form whose explicit operator's pattern is rebuilt as well
MG_REGROUP_CASES = {
    "regroup_plain":         (dict(mg_smoothed_levels=0, mg_dense_max_nodes=16, mg_passes=2), dict(passes=2, dense_max=16, smoothed_levels=0, explicit=False), 3),
    "regroup_smoothed_expl": (dict(mg_smoothed_levels=1, mg_dense_max_nodes=16, mg_passes=2, mg_explicit_transfer=1), dict(passes=2, dense_max=16, smoothed_levels=1, explicit=True), 3),
}


def model_arguments(margs):
    """the arguments of a case for precond_model.multigrid (passes and dense_max shape the hierarchy, not the model)"""
    return {k: v for k, v in margs.items() if k not in ("passes", "dense_max")}


# the PCG forms that actually run (tests/test_gpu_precond_operator.py pins their iterates x_k to the model, tests/pcg_bits_cases.py records their bits)
BJ, TL, MG = capi.PRECOND_BLOCK_JACOBI, capi.PRECOND_TWO_LEVEL, capi.PRECOND_MULTIGRID
MG1 = dict(MG_BASE, **MG_CASES["one_sparse"][0])
MG3 = dict(MG_BASE, **MG_CASES["three_levels"][0])
FORMS = {
    # label: (graph, options, preconditioner, single-reduction form expected, multigrid case)
    "block-Jacobi single-reduction":    ("bj300", dict(coarse_aggregates=0), BJ, 1, None),
    "block-Jacobi classic (tolerance)": ("bj300", dict(coarse_aggregates=0, cg_rel_tolerance=1e-12), BJ, 0, None),
    "block-Jacobi classic (option)":    ("bj300", dict(coarse_aggregates=0, cg_single_reduction=0), BJ, 0, None),
    "block-Jacobi block-CSR":           ("bj300", dict(coarse_aggregates=0, linear_solver=0), BJ, 0, None),
    "two-level fused sr_coarse":        ("tl600", dict(coarse_aggregates=64), TL, 1, None),
    "two-level fused classic_coarse":   ("tl600", dict(coarse_aggregates=64, cg_single_reduction=0), TL, 0, None),
    "two-level unfused m=75":           ("tl600", dict(coarse_aggregates=8, coarse_min_radius=0.0), TL, 0, None),
    "two-level unfused block-CSR":      ("tl600", dict(coarse_aggregates=64, linear_solver=0), TL, 0, None),
    "multigrid restricted update":      ("mg640", MG1, MG, 1, "one_sparse"),
    "multigrid restricted classic":     ("mg640", dict(MG1, cg_single_reduction=0), MG, 0, "one_sparse"),
    "multigrid split update":           ("mg640", MG3, MG, 1, "three_levels"),      # two sparse levels: three launches can carry riders, choose_split takes two of them
    "multigrid block-CSR":              ("mg640", dict(MG1, linear_solver=0), MG, 0, "one_sparse"),
}
KS = (1, 2, 3, 6)
# ... and of the new paths, in a table of their own (FORMS is what tests/pcg_bits_cases.py records against its golden):
# label: (graph, options, single-reduction form expected, case of MG_PATH_CASES or MG_REGROUP_CASES, regroup: the handle solves from state A first and is pinned at state B)
PATH_FORMS = {
    "multigrid rescaled explicit":  ("mgyaw640", dict(MG_BASE, **MG_PATH_CASES["rescaled_smoothed_expl"][1]), 1, "rescaled_smoothed_expl", False),      # the form that runs by default: single reduction, explicit transfer
    "multigrid regrouped explicit": ("mg640", dict(MG_BASE, **MG_REGROUP_CASES["regroup_smoothed_expl"][0]), 1, "regroup_smoothed_expl", True),
}


def limit_margin(model, omega=pm.OMEGA):
    """distance of the smoother-limit estimate of every sparse level from the limit the rescaling starts at"""
    return min([abs(omega * e - pm.SMOOTHER_LIMIT) for e in model["lam_est"]] or [1.0])
