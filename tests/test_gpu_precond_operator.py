"""GPU: the block-Jacobi, two-level and multigrid preconditioners and the fused PCG iteration forms AS LINEAR OPERATORS, against the dense fp64 model of
tests/precond_model.py (checked on the CPU, with its teeth, in tests/test_precond_model.py).

PCG hides a wrong preconditioner: with any M^-1 it ends at an x with a small residual, so trajectory tests stay green and only iterations are lost.  Here the dense M_dev
is extracted through pgo_apply_preconditioner (ONE batched call with R = I) and compared entry by entry; the iteration forms that actually run are pinned through the iterate
x_k of a k-step PCG (pgo_get_linear_solution) against textbook PCG with the model's M^-1.

All norms are max-norms relative to |M_64|.  Tolerances come from the model alone: e_ref = |M_32 - M_64| is what rounding the device's fp32 objects (level matrices, R^T,
dense inverses, packed block-Jacobi factors) costs IN THE MODEL; the device, which rounds at other points (Cholesky factors instead of inverses, Gauss-Jordan order), gets
8 e_ref + 1e-10, and 8 e_ref <= 1e-3 is asserted for every case so that the bound stays a bound.  Symmetry: exact transposes in fp32 with fp64 accumulation leave fp64 noise
(~1e-13); one asymmetric fp32 rounding would show at 6e-8 or more: 1e-10 separates the two.

The multigrid is also compared on the paths the library takes by default on real graphs (tests/precond_cases.py: MG_PATH_CASES, MG_REGROUP_CASES): a hierarchy one of whose
levels gets the smoother's safety rescaling, the smoothed keyframe transition, and the hierarchy a handle installs when its next solve starts from other switch values (regroup).

Every test prints its figures (`PRECOND ...`) before it asserts; profiles/precond_operator_check.txt records them.  PRECOND_REPORT_EIGENVALUES=1 in the environment adds the
smallest eigenvalue of sym(M_dev) to the line (seconds per case: not part of the suite's run)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from solve_keyframe_pose_graph_amd import capi
from tests import precond_cases as pc
from tests import precond_model as pm
from tests import solve_digest, util
from tests.precond_child import linear_iterate

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BJ, TL, MG = capi.PRECOND_BLOCK_JACOBI, capi.PRECOND_TWO_LEVEL, capi.PRECOND_MULTIGRID
PGO_ERR_INVALID_ARG, PGO_ERR_STATE = -1, -5


def open_solve(graph, constant=(), drop_last=0, **opt):
    g = pc.graph(graph, drop_last)
    P = util.pgo_problem(g, True, **opt)
    if constant:
        P.set_nodes_constant(list(constant))
    q, t, s = pc.state(g)
    P.solve_begin(q, t, s)
    return P


def dense_operator(P, which, radius, lin):
    """M_dev over ALL keyframes: one batched call with R = I (column v of M is the image of unit vector v)"""
    return P.apply_preconditioner(which, np.eye(6 * lin.N), radius).T.copy()


def is_positive_definite(M):
    try:
        np.linalg.cholesky(0.5 * (M + M.T))
        return True
    except np.linalg.LinAlgError:
        return False


def check_operator(label, radius, M_full, lin, m64, m32, against_model=True):
    """the model-free assertions on M_dev and, against the model, |M_dev - M_64| <= 8 e_ref + 1e-10; returns M_dev over the free keyframes"""
    outside = np.setdiff1d(np.arange(6 * lin.N), lin.rows)
    Md = M_full[np.ix_(lin.rows, lin.rows)]
    ref = m64["M"]
    norm = pm.maxnorm(ref)
    asym = pm.maxnorm(Md - Md.T) / norm
    e_ref = pm.maxnorm(m32["M"] - ref) / norm
    err = pm.maxnorm(Md - ref) / norm
    pd = is_positive_definite(Md)
    extra = ""
    if os.environ.get("PRECOND_REPORT_EIGENVALUES") == "1":
        import scipy.linalg
        extra = " lambda_min %.3e" % scipy.linalg.eigvalsh(0.5 * (Md + Md.T), subset_by_index=[0, 0])[0]
    if against_model:
        print("PRECOND operator %-28s radius %.0e  n %5d  e_ref %.3e  |M_dev - M_64| %.3e  (|M_dev - M_32| %.3e)  asymmetry %.3e  positive definite %s%s" %
              (label, radius, len(Md), e_ref, err, pm.maxnorm(Md - m32["M"]) / norm, asym, pd, extra))
    else:
        print("PRECOND operator %-28s radius %.0e  n %5d  (no model)  asymmetry %.3e relative to |D^-1|  positive definite %s%s" % (label, radius, len(Md), asym, pd, extra))
    assert np.all(M_full[outside, :] == 0.0) and np.all(M_full[:, outside] == 0.0)      # constant and unreferenced keyframes: exactly zero
    assert asym <= 1e-10
    assert pd
    if against_model:
        assert 8 * e_ref <= 1e-3                                                        # the condition that keeps the bound honest
        assert err <= 8 * e_ref + 1e-10
    return Md


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# block-Jacobi and the two-level method
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", pc.RADII)
def test_block_jacobi_operator(radius):
    lin = pc.linearisation("bj300")
    A, _ = pc.system("bj300", radius)
    P = open_solve("bj300")
    M = dense_operator(P, BJ, radius, lin)
    P.solve_end(); P.close()
    check_operator("block-Jacobi N=300", radius, M, lin, dict(M=pm.block_jacobi(A)), dict(M=pm.block_jacobi(A, fp32=True)))


TWO_LEVEL_CASES = {
    # label: (graph, constant, unreferenced at the end, options, m)
    "one aggregate per keyframe": ("tl200", (), 0, dict(), 1),
    "fused m=10 N=600":           ("tl600", (), 0, dict(coarse_aggregates=64), 10),
    "fused m=10 N=601":           ("tl601", (), 0, dict(coarse_aggregates=64), 10),      # a last aggregate of one keyframe
    "unfused m=75":               ("tl600", (), 0, dict(coarse_aggregates=8, coarse_min_radius=0.0), 75),
    "constant keyframes":         ("tl600", pc.CONSTANT_TL600, 3, dict(coarse_aggregates=64), 10),      # a whole aggregate, half of another, three unreferenced keyframes at the end
}


@pytest.mark.parametrize("radius", pc.RADII)
@pytest.mark.parametrize("label", sorted(TWO_LEVEL_CASES))
def test_two_level_operator(label, radius):
    graph, constant, drop, opt, m = TWO_LEVEL_CASES[label]
    lin = pc.linearisation(graph, constant, drop)
    A, _ = pc.system(graph, radius, constant, drop)
    assert pm.two_level_aggregates(lin.N, opt.get("coarse_aggregates", 768))[0] == m
    m64, m32 = pm.two_level(lin, A, m), pm.two_level(lin, A, m, fp32=True)
    assert is_positive_definite(m32["Ac_inv"])                                          # the radius is one at which the model's fp32 Ac^-1 is still positive definite
    P = open_solve(graph, constant, drop, **opt)
    M = dense_operator(P, TL, radius, lin)
    D = dense_operator(P, BJ, radius, lin) if m > 1 else None
    P.solve_end(); P.close()
    Md = check_operator("two-level " + label, radius, M, lin, m64, m32)
    # the coarse correction is a projector in the A inner product: C A C = C, to 10 x the defect of the model's fp32 form
    C_dev = Md - D[np.ix_(lin.rows, lin.rows)] if m > 1 else Md
    C32 = m32["C"]
    defect_model = pm.maxnorm(C32 @ A @ C32 - C32) / pm.maxnorm(C32)
    defect_dev = pm.maxnorm(C_dev @ A @ C_dev - C_dev) / pm.maxnorm(C32)
    print("PRECOND projector %-27s radius %.0e  |C A C - C| device %.3e  model fp32 %.3e" % (label, radius, defect_dev, defect_model))
    assert defect_dev <= 10 * defect_model


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# multigrid
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def device_hierarchy(P):
    """(agg0, parents of every sparse level) of the hierarchy the device has installed"""
    agg0 = P.mg_level_parents(0)
    parents, level = [], 1
    while True:
        try:
            parents.append(P.mg_level_parents(level))
        except capi.PgoError as e:
            assert e.code == PGO_ERR_INVALID_ARG
            return agg0, parents
        level += 1


def mg_models(lin, A, agg0, parents, margs):
    kw = dict(smoothed_levels=margs["smoothed_levels"], explicit=margs["explicit"])
    m64, m32 = pm.multigrid(lin, A, agg0, parents, **kw), pm.multigrid(lin, A, agg0, parents, fp32=True, **kw)
    # the smoother limit (rescaling from omega lambda > 1.75) is inactive and clear of its threshold on this graph: the model and the device take the same branch
    assert not m64["limit_active"] and not m32["limit_active"] and pc.limit_margin(m64) >= 0.01 and pc.limit_margin(m32) >= 0.01, (m64["lam_est"], m32["lam_est"])
    return m64, m32


def mg_operator(case, radius, constant=()):
    opt, margs, n_levels = pc.MG_CASES[case]
    lin = pc.linearisation("mg640", constant)
    A, _ = pc.system("mg640", radius, constant)
    P = open_solve("mg640", constant, **dict(pc.MG_BASE, **opt))
    M = dense_operator(P, MG, radius, lin)
    agg0, parents = device_hierarchy(P)
    P.solve_end(); P.close()
    assert len(parents) + 1 == n_levels, [len(p) for p in parents]
    assert np.array_equal(agg0 >= 0, lin.free)
    m64, m32 = mg_models(lin, A, agg0, parents, margs)
    return lin, M, m64, m32


@pytest.mark.parametrize("radius", pc.RADII)
@pytest.mark.parametrize("case", ["dense", "one_sparse", "three_levels"])
def test_multigrid_operator(case, radius):
    lin, M, m64, m32 = mg_operator(case, radius)
    check_operator("multigrid " + case, radius, M, lin, m64, m32)


@pytest.mark.parametrize("radius", pc.RADII)
def test_multigrid_smoothed_operator_implicit_and_explicit(radius):
    """both forms of the smoothed transition against the model AND against each other (the same operator up to where R^T is rounded)"""
    lin, Mi, m64, m32i = mg_operator("smoothed_impl", radius)
    _, Me, m64e, m32e = mg_operator("smoothed_expl", radius)
    Mdi = check_operator("multigrid smoothed implicit", radius, Mi, lin, m64, m32i)
    Mde = check_operator("multigrid smoothed explicit", radius, Me, lin, m64e, m32e)
    norm = pm.maxnorm(m64["M"])
    e_i, e_e = pm.maxnorm(m32i["M"] - m64["M"]) / norm, pm.maxnorm(m32e["M"] - m64e["M"]) / norm
    diff = pm.maxnorm(Mdi - Mde) / norm
    print("PRECOND smoothed implicit vs explicit  radius %.0e  |M_impl - M_expl| %.3e  (e_ref %.3e / %.3e)" % (radius, diff, e_i, e_e))
    assert diff <= 8 * (e_i + e_e) + 1e-10


@pytest.mark.parametrize("radius", pc.RADII)
def test_multigrid_operator_with_constant_keyframes(radius):
    lin, M, m64, m32 = mg_operator("one_sparse", radius, pc.CONSTANT_MG640)
    assert lin.free.sum() == 610
    check_operator("multigrid constant run", radius, M, lin, m64, m32)


@pytest.mark.parametrize("radius", pc.RADII)
def test_multigrid_smoothed_keyframe_transition_is_symmetric_positive_definite(radius):
    """mg_smoothed_fine = 1: model-free properties only (against the model: test_multigrid_smoothed_keyframe_transition_operator)"""
    lin = pc.linearisation("mg640")
    A, _ = pc.system("mg640", radius)
    P = open_solve("mg640", **dict(pc.MG_BASE, mg_smoothed_fine=1, mg_smoothed_levels=1, mg_dense_max_nodes=64))
    M = dense_operator(P, MG, radius, lin)
    P.solve_end(); P.close()
    D = pm.block_jacobi(A)
    check_operator("multigrid smoothed keyframes", radius, M, lin, dict(M=D), dict(M=D), against_model=False)


# ---- the paths the library takes by default on real graphs: the smoother's safety rescaling, the smoothed keyframe transition, a hierarchy after a regroup ----
def mg_models_expecting(lin, A, agg0, parents, margs, rescaled):
    """mg_models for the cases whose smoother limit IS active on some level: every sparse level of the DEVICE's hierarchy lies on the side of the limit the case names,
    and clear of it by the same 0.01 — level by level, so the model and the device take the same branch on each"""
    kw = pc.model_arguments(margs)
    m64, m32 = pm.multigrid(lin, A, agg0, parents, **kw), pm.multigrid(lin, A, agg0, parents, fp32=True, **kw)
    for m in (m64, m32):
        assert m["rescaled"] == list(rescaled) and all(pc.limit_margin(dict(lam_est=[e])) >= 0.01 for e in m["lam_est"]), (m64["lam_est"], m32["lam_est"])
    return m64, m32


def path_operator(case, radius):
    graph, opt, margs, n_levels, rescaled = pc.MG_PATH_CASES[case]
    lin = pc.linearisation(graph)
    A, _ = pc.system(graph, radius)
    P = open_solve(graph, **dict(pc.MG_BASE, **opt))
    M = dense_operator(P, MG, radius, lin)
    agg0, parents = device_hierarchy(P)
    P.solve_end(); P.close()
    assert len(parents) + 1 == n_levels, [len(p) for p in parents]
    assert np.array_equal(agg0 >= 0, lin.free)
    m64, m32 = mg_models_expecting(lin, A, agg0, parents, margs, rescaled)
    return lin, M, m64, m32


@pytest.mark.parametrize("radius", pc.RADII)
@pytest.mark.parametrize("case", ["rescaled_plain", "fine_rescaled"])
def test_multigrid_rescaled_operator(case, radius):
    """one sparse level's smoother is rescaled (mg_rescale_dinv_kernel) and the other's is not — rescaled_plain: level 2; fine_rescaled: level 1 = Ps_0^T A Ps_0, whose
    unrescaled smoother would leave M^-1 indefinite, with the smoothed transition above it formed from the rescaled Dinv"""
    lin, M, m64, m32 = path_operator(case, radius)
    check_operator("multigrid " + case, radius, M, lin, m64, m32)


@pytest.mark.parametrize("radius", pc.RADII)
def test_multigrid_rescaled_smoothed_operator_implicit_and_explicit(radius):
    """a smoothed transition below the rescaled level, both forms, against the model and against each other"""
    lin, Mi, m64, m32i = path_operator("rescaled_smoothed_impl", radius)
    _, Me, m64e, m32e = path_operator("rescaled_smoothed_expl", radius)
    Mdi = check_operator("multigrid rescaled_smoothed_impl", radius, Mi, lin, m64, m32i)
    Mde = check_operator("multigrid rescaled_smoothed_expl", radius, Me, lin, m64e, m32e)
    norm = pm.maxnorm(m64["M"])
    e_i, e_e = pm.maxnorm(m32i["M"] - m64["M"]) / norm, pm.maxnorm(m32e["M"] - m64e["M"]) / norm
    diff = pm.maxnorm(Mdi - Mde) / norm
    print("PRECOND rescaled implicit vs explicit  radius %.0e  |M_impl - M_expl| %.3e  (e_ref %.3e / %.3e)" % (radius, diff, e_i, e_e))
    assert diff <= 8 * (e_i + e_e) + 1e-10


@pytest.mark.parametrize("radius", pc.RADII)
def test_multigrid_smoothed_keyframe_transition_operator(radius):
    """mg_smoothed_fine = 1 against the model: Ps_0 = (I - w_p D^-1 A) P_0 in both orientations, level 1 = Ps_0^T A Ps_0"""
    lin, M, m64, m32 = path_operator("fine640", radius)
    check_operator("multigrid fine640", radius, M, lin, m64, m32)


def same_hierarchy(a, b):
    return np.array_equal(a[0], b[0]) and len(a[1]) == len(b[1]) and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))


def entries_moved(a, b):
    return [int((x != y).sum()) if len(x) == len(y) else -1 for x, y in zip([a[0]] + list(a[1]), [b[0]] + list(b[1]))]


@pytest.mark.parametrize("radius", pc.RADII)
@pytest.mark.parametrize("case", sorted(pc.MG_REGROUP_CASES))
def test_multigrid_operator_after_a_regroup(case, radius):
    """One handle opens a solve at state A, closes it and opens the next at state B (the outlier loop closures switched off): regroup_if_moved "for the new start" rebuilds
    the hierarchy from the cache and installs it (regroup_commit, mg_install).  What is installed then is what a fresh handle installs at B, and the operators built on the
    re-installed pools are those of the new aggregates: M_dev against the model built from the regrouped handle's own parents at B's linearisation."""
    opt, margs, n_levels = pc.MG_REGROUP_CASES[case]
    g = pc.graph("mg640")
    opts = dict(pc.MG_BASE, **opt)
    lin = pc.linearisation("mg640", regroup="B")
    A, _ = pc.system("mg640", radius, regroup="B")
    P = util.pgo_problem(g, True, **opts)
    P.solve_begin(*pc.state(g))
    at_a = device_hierarchy(P)
    P.solve_end()
    P.solve_begin(*pc.state(g, "B"))
    regrouped = device_hierarchy(P)
    M = dense_operator(P, MG, radius, lin)
    P.solve_end(); P.close()
    F = util.pgo_problem(g, True, **opts)
    F.solve_begin(*pc.state(g, "B"))
    fresh = device_hierarchy(F)
    F.solve_end(); F.close()
    print("PRECOND regroup %-24s radius %.0e  entries moved per level A -> B %s  regrouped vs fresh at B %s" % (case, radius, entries_moved(at_a, regrouped), entries_moved(regrouped, fresh)))
    assert not same_hierarchy(at_a, regrouped)
    assert same_hierarchy(regrouped, fresh)
    assert len(regrouped[1]) + 1 == n_levels and np.array_equal(regrouped[0] >= 0, lin.free)
    m64, m32 = mg_models_expecting(lin, A, regrouped[0], regrouped[1], margs, (False,) * (n_levels - 1))
    check_operator("multigrid " + case, radius, M, lin, m64, m32)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# the forms that actually run: x_k of a k-step PCG
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
FORMS, KS = pc.FORMS, pc.KS      # (the table lives in tests/precond_cases.py: tests/pcg_bits_cases.py records the bits of the same forms)


def reference_iterates(graph, opt, precond, mg_case, radius, handle_for_hierarchy, kmax):
    """([x_1 .. x_kmax] with M_64, the same with M_32, lin)"""
    lin = pc.linearisation(graph)
    A, b = pc.system(graph, radius)
    if precond == BJ:
        M64, M32 = pm.block_jacobi(A), pm.block_jacobi(A, fp32=True)
    elif precond == TL:
        m = pm.two_level_aggregates(lin.N, opt["coarse_aggregates"])[0]
        M64, M32 = pm.two_level(lin, A, m)["M"], pm.two_level(lin, A, m, fp32=True)["M"]
    else:
        agg0, parents = device_hierarchy(handle_for_hierarchy)
        m64, m32 = mg_models(lin, A, agg0, parents, pc.MG_CASES[mg_case][1])
        M64, M32 = m64["M"], m32["M"]
    return pm.pcg(A, b, M64, kmax), pm.pcg(A, b, M32, kmax), lin


def check_iterate(label, radius, k, x, it, lin, x64, x32, precond, sr):
    outside = np.setdiff1d(np.arange(6 * lin.N), lin.rows)
    xd = x[lin.rows]
    tol = 8 * pm.maxnorm(x32[k - 1] - x64[k - 1]) + 1e-9 * pm.maxnorm(x64[k - 1])
    dev = pm.maxnorm(xd - x64[k - 1])
    print("PRECOND iterate %-34s radius %.0e  k %d  |x_k - x_k(M_64)| %.3e  tolerance %.3e  |x_k| %.3e" % (label, radius, k, dev, tol, pm.maxnorm(x64[k - 1])))
    assert it.cg_iterations == k and it.preconditioner == precond and it.single_reduction == sr, (it.cg_iterations, it.preconditioner, it.single_reduction)
    assert np.all(x[outside] == 0.0)
    assert dev <= tol


@pytest.mark.parametrize("radius", pc.RADII)
@pytest.mark.parametrize("label", sorted(FORMS))
def test_iterates_of_the_forms_that_run(label, radius):
    graph, opt, precond, sr, mg_case = FORMS[label]
    P, got = None, {}
    for k in KS:
        x, it, P = linear_iterate(graph, k, radius, handle=P, **opt)
        got[k] = (x, it)
    x64, x32, lin = reference_iterates(graph, opt, precond, mg_case, radius, P, max(KS))
    P.close()
    for k in KS:
        check_iterate(label, radius, k, got[k][0], got[k][1], lin, x64, x32, precond, sr)


@pytest.mark.parametrize("radius", pc.RADII)
@pytest.mark.parametrize("label", sorted(pc.PATH_FORMS))
def test_iterates_of_the_new_paths(label, radius):
    """x_k of the form that runs by default (single reduction, explicit transfer) on a hierarchy with a rescaled level, and on a handle that regrouped at this solve's start"""
    graph, opt, sr, case, regroup = pc.PATH_FORMS[label]
    P, got = None, {}
    if regroup:      # a solve from state A first: the first of the solves from B below then starts with the regroup, the later ones find the hierarchy already B's
        _, _, P = linear_iterate(graph, 1, radius, regroup="A", **opt)
        at_a = device_hierarchy(P)
    for k in KS:
        x, it, P = linear_iterate(graph, k, radius, handle=P, regroup="B" if regroup else None, **opt)
        got[k] = (x, it)
    agg0, parents = device_hierarchy(P)
    P.close()
    lin = pc.linearisation(graph, regroup="B" if regroup else None)
    A, b = pc.system(graph, radius, regroup="B" if regroup else None)
    if regroup:
        assert not same_hierarchy(at_a, (agg0, parents))
        margs, rescaled = pc.MG_REGROUP_CASES[case][1], (False,) * (pc.MG_REGROUP_CASES[case][2] - 1)
    else:
        margs, rescaled = pc.MG_PATH_CASES[case][2], pc.MG_PATH_CASES[case][4]
    m64, m32 = mg_models_expecting(lin, A, agg0, parents, margs, rescaled)
    x64, x32 = pm.pcg(A, b, m64["M"], max(KS)), pm.pcg(A, b, m32["M"], max(KS))
    for k in KS:
        check_iterate(label, radius, k, got[k][0], got[k][1], lin, x64, x32, MG, sr)


def test_iterate_out_of_a_captured_chunk():
    """PGO_DEBUG_GRAPH_AFTER=2 in a process of its own, chunks of two iterations: iterations 2 .. 7 of an 8-step PCG are replays of the captured chunk"""
    radius, k = pc.RADII[0], 8
    opt = dict(coarse_aggregates=64, cg_check_every=2, verbosity=2)
    env = dict(os.environ, PGO_ENABLE_DEBUG_HOOKS="1", PGO_DEBUG_GRAPH_AFTER="2")
    arg = json.dumps(dict(graph="tl600", k=k, radius=radius, opt=opt))
    out = subprocess.run([sys.executable, "-m", "tests.precond_child", arg], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "PCG chunk of 2 iterations (preconditioner 1) captured" in out.stderr, out.stderr[-2000:]
    rec = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("ITERATE ")][-1][len("ITERATE "):])
    x = np.array([float.fromhex(v) for v in rec["x"]])
    x64, x32, lin = reference_iterates("tl600", opt, TL, None, radius, None, k)

    class It:
        cg_iterations, preconditioner, single_reduction = rec["cg_iterations"], rec["preconditioner"], rec["single_reduction"]
    check_iterate("two-level fused, captured chunk", radius, k, x, It, lin, x64, x32, TL, 1)


def test_converged_iterate_solves_the_system():
    """x of a converged PCG against numpy.linalg.solve(A, b): pins b (the reduced negative gradient) and the stopping rule besides the operator"""
    radius = pc.RADII[0]
    x, it, P = linear_iterate("tl600", 5000, radius, coarse_aggregates=64, cg_rel_tolerance=1e-11)
    P.close()
    lin = pc.linearisation("tl600")
    A, b = pc.system("tl600", radius)
    ref = np.linalg.solve(A, b)
    err = pm.maxnorm(x[lin.rows] - ref) / pm.maxnorm(ref)
    print("PRECOND converged two-level fused  radius %.0e  %d iterations  |x - A^-1 b| / |A^-1 b| %.3e" % (radius, it.cg_iterations, err))
    assert it.cg_iterations < 5000 and err <= 1e-7


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# contract
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def raw_apply(P, which, radius, n_vec, R, Z):
    import ctypes as C
    dp = C.POINTER(C.c_double)
    return P.lib.pgo_apply_preconditioner(P.h, C.c_int32(which), C.c_double(radius), C.c_int64(n_vec), R.ctypes.data_as(dp) if R is not None else None, Z.ctypes.data_as(dp) if Z is not None else None)


def test_hook_error_paths():
    g = pc.graph("tl200")
    q, t, s = pc.state(g)
    n6 = 6 * g.n_poses
    R, Z = np.zeros(n6), np.zeros(n6)
    P = util.pgo_problem(g, True)
    # before a solve is open
    assert raw_apply(P, BJ, 0.0, 1, R, Z) == PGO_ERR_STATE and b"open solve" in P.lib.pgo_last_error(P.h)
    with pytest.raises(capi.PgoError) as e:
        P._shape = (g.n_poses, len(s)); P.linear_solution()
    assert e.value.code == PGO_ERR_STATE
    with pytest.raises(capi.PgoError) as e:
        P.mg_level_parents(0)
    assert e.value.code == PGO_ERR_STATE
    P.solve_begin(q, t, s)
    # invalid arguments
    for which, radius, n_vec, r, z in ((7, 0.0, 1, R, Z), (-1, 0.0, 1, R, Z), (BJ, 0.0, 0, R, Z), (BJ, float("nan"), 1, R, Z), (BJ, float("inf"), 1, R, Z), (BJ, 0.0, 1, None, Z), (BJ, 0.0, 1, R, None)):
        assert raw_apply(P, which, radius, n_vec, r, z) == PGO_ERR_STATE and b"invalid argument" in P.lib.pgo_last_error(P.h)
    # a preconditioner this graph does not have; no PCG has run yet
    assert raw_apply(P, MG, 0.0, 1, R, Z) == PGO_ERR_STATE and b"no multigrid hierarchy" in P.lib.pgo_last_error(P.h)
    with pytest.raises(capi.PgoError) as e:
        P.linear_solution()
    assert e.value.code == PGO_ERR_STATE
    with pytest.raises(capi.PgoError) as e:
        P.mg_level_parents(0)
    assert e.value.code == PGO_ERR_STATE
    # radius <= 0 means the current radius, and the call leaves the radius alone
    rng = np.random.default_rng(0)
    r1 = rng.normal(size=n6)
    z_cur = P.apply_preconditioner(TL, r1, 0.0)
    z_1e4 = P.apply_preconditioner(TL, r1, 1e4)      # (the initial radius)
    z_1e6 = P.apply_preconditioner(TL, r1, 1e6)
    assert np.array_equal(z_cur, z_1e4) and not np.array_equal(z_cur, z_1e6)
    assert np.array_equal(P.apply_preconditioner(TL, r1, -1.0), z_cur)
    P.solve_end(); P.close()
    # a graph with a hierarchy has no two-level aggregates; its coarsest level has no parents
    P = open_solve("mg640", **dict(pc.MG_BASE, **pc.MG_CASES["one_sparse"][0]))
    n6 = 6 * 640
    assert raw_apply(P, TL, 0.0, 1, np.zeros(n6), np.zeros(n6)) == PGO_ERR_STATE and b"no two-level aggregates" in P.lib.pgo_last_error(P.h)
    assert len(P.mg_level_parents(0)) == 640 and len(P.mg_level_parents(1)) == 80
    import ctypes as C
    n = C.c_int64(0)
    assert P.lib.pgo_mg_level_parents(P.h, C.c_int32(2), None, C.c_int64(0), C.byref(n)) == PGO_ERR_INVALID_ARG
    short = np.zeros(10, np.int32)
    assert P.lib.pgo_mg_level_parents(P.h, C.c_int32(0), short.ctypes.data_as(C.POINTER(C.c_int32)), C.c_int64(10), C.byref(n)) == PGO_ERR_INVALID_ARG and n.value == 640
    P.solve_end(); P.close()


def test_hooks_refuse_a_handle_with_a_communicator():
    g = pc.graph("tl200")
    P = util.pgo_problem(g, True)
    P.comm_init_custom(0, 1, lambda buf, count, op, stream: 0)
    n6 = 6 * g.n_poses
    assert raw_apply(P, BJ, 0.0, 1, np.zeros(n6), np.zeros(n6)) == PGO_ERR_STATE and b"communicator" in P.lib.pgo_last_error(P.h)
    P._shape = (g.n_poses, g.n_loops)
    for call in (P.linear_solution, lambda: P.mg_level_parents(0)):
        with pytest.raises(capi.PgoError) as e:
            call()
        assert e.value.code == PGO_ERR_STATE and "communicator" in str(e.value)
    P.comm_destroy(); P.close()


@pytest.mark.parametrize("name,opt,hooks", [("C1F5", dict(), (BJ, TL)), ("G6000", dict(), (BJ, MG))])
def test_a_handle_the_hooks_were_used_on_solves_like_a_fresh_one(name, opt, hooks):
    """hooks between solve_begin and solve_end (no LM step), then a solve on the same handle: every output array and the whole iteration log equal a fresh handle's, bit for bit"""
    fresh = solve_digest.digest(name, **opt)
    g, switchable = solve_digest.graph(name)
    q, t, s = util.initial_state(g, switchable)
    P = util.pgo_problem(g, switchable, **opt)
    P.solve_begin(q, t, s)
    rng = np.random.default_rng(1)
    R = rng.normal(size=(3, 6 * g.n_poses))
    for which in hooks:
        for radius in (0.0, 1e7):
            assert np.isfinite(P.apply_preconditioner(which, R, radius)).all()
    if MG in hooks:
        assert len(P.mg_level_parents(0)) == g.n_poses
    P.solve_end()
    used = solve_digest.digest(name, handle=P, **opt)
    P.close()
    assert used == fresh
