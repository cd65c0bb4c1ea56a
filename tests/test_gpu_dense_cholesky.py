"""GPU: the exact dense linear solver (pgo_options.linear_solver = PGO_LINEAR_DENSE_CHOLESKY; csrc/pgo_dense.hip).

  1. the kernels alone (pgo_dense_spd_solve) against numpy;  2. an LM step's C.x is the exact solution of the model's system (tests/precond_cases.py), measured against the
  block-CSR PCG run to the floor of its accuracy;  3. the same on a graph with robust loop closures;  4. solve trajectories against the CPU checker with every other option
  at its default;  5. determinism;  6. a failed factorisation is an invalid step, not a failed solve;  7. the contract of the option and of the hooks.

u = 2^-53, eta(A, b, x) = |b - A x|_inf / (|A|_inf |x|_inf + |b|_inf) with the residual formed in extended precision, n the matrix order.  The bound eta <= n u is the
first-order size of the rounding bound of an n-term fp64 inner product in any order: derived, not measured.  Every test prints its figures (`DENSE ...`) before it
asserts; profiles/dense_cholesky_check.txt records them."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from solve_keyframe_pose_graph_amd import capi, graphgen
from tests import precond_cases as pc
from tests import util
from tests.precond_child import linear_iterate

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
DENSE = capi.LINEAR_DENSE_CHOLESKY
PGO_ERR_INVALID_ARG, PGO_ERR_STATE = -1, -5
# the parent's most accurate solver on the same system: the classic block-CSR PCG, block-Jacobi alone, run to the floor of its attainable accuracy
PCG_FLOOR = dict(linear_solver=0, coarse_aggregates=0, cg_rel_tolerance=1e-13)
PCG_MAX_ITERATIONS = 20000


def eta(A, b, x):
    r = b.astype(np.longdouble) - A.astype(np.longdouble) @ x.astype(np.longdouble)
    return float(np.abs(r).max() / (np.abs(A).sum(axis=1).max() * np.abs(x).max() + np.abs(b).max()))


def spd(n):
    """as tests/test_gpu_coarse.py::test_dense_inverse_against_numpy builds them"""
    rng = np.random.default_rng(n)
    B = rng.standard_normal((n, max(8, n // 2)))
    A = B @ B.T + np.diag(rng.uniform(1e-3, 1.0, n))
    return 0.5 * (A + A.T), rng.standard_normal(n)


def direct_records(sm):
    """every logged iteration >= 1 is a dense step"""
    for k in range(1, sm.num_logged):
        it = sm.iterations[k]
        assert it.cg_iterations == 0 and it.cg_iterations_multigrid == 0 and it.single_reduction == 0 and it.cg_residual == 0.0, k
        assert it.preconditioner == capi.PRECOND_DIRECT, (k, it.preconditioner)
    assert sm.cg_iterations == 0 and sm.pcg_retries == 0


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 1. the kernels alone
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 96, 200, 1088, 2048])      # one tile; padding inside the second tile; 200; 17 tiles (an odd count); 32 tiles
def test_dense_spd_solve_against_numpy(n):
    A, b = spd(n)
    P = capi.Problem()
    x, ms = P.dense_spd_solve(A, b)
    x2, _ = P.dense_spd_solve(A, b)
    P.close()
    e, e_ref = eta(A, b, x), eta(A, b, np.linalg.solve(A, b))
    print("DENSE kernels n %4d  eta %.3e = %.2f u  (numpy.linalg.solve: %.2f u; bound n u = %.3e)  %.3f ms" % (n, e, e / U, e_ref / U, n * U, ms))
    assert e <= n * U
    assert np.array_equal(x, x2)      # no atomics, fixed summation order: the same bits


def test_dense_spd_solve_reports_an_indefinite_matrix_and_a_nan():
    P = capi.Problem()
    A = np.eye(128); A[70, 70] = -1.0
    with pytest.raises(capi.PgoError) as e:
        P.dense_spd_solve(A, np.ones(128))
    assert e.value.code == -7      # PGO_ERR_NUMERIC
    A = np.eye(128); A[100, 3] = A[3, 100] = np.nan
    with pytest.raises(capi.PgoError):
        P.dense_spd_solve(A, np.ones(128))
    x, _ = P.dense_spd_solve(np.eye(128), np.ones(128))      # ... and the handle goes on working
    assert np.array_equal(x, np.ones(128))
    P.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 2. the step is the exact solution
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
STEP_CASES = [("tl200", (), 0), ("tl600", (), 0), ("tl600", pc.CONSTANT_TL600, 3)]      # the last: identity rows in the middle of the matrix and at its end


@pytest.mark.parametrize("radius", pc.RADII)
@pytest.mark.parametrize("name,constant,drop_last", STEP_CASES)
def test_the_step_is_the_exact_solution(name, constant, drop_last, radius):
    lin = pc.linearisation(name, constant, drop_last)
    A, b = pc.system(name, radius, constant, drop_last)
    n = A.shape[0]
    x, it, P = linear_iterate(name, 1, radius, constant, drop_last, linear_solver=DENSE)
    P.close()
    assert it.step_is_valid and it.cg_iterations == 0 and it.preconditioner == capi.PRECOND_DIRECT and it.cg_residual == 0.0 and it.single_reduction == 0
    outside = np.ones(len(x), bool); outside[lin.rows] = False
    assert np.all(x[outside] == 0.0)
    xp, itp, P = linear_iterate(name, PCG_MAX_ITERATIONS, radius, constant, drop_last, **PCG_FLOOR)
    P.close()
    e_dense, e_pcg = eta(A, b, x[lin.rows]), eta(A, b, xp[lin.rows])
    print("DENSE step %s constant %d drop_last %d radius %.0e  n %d  eta_dense %.3e = %.2f u  eta_pcg %.3e = %.2f u (%d iterations)  bound max(4 eta_pcg, n u) = %.3e"
          % (name, len(constant), drop_last, radius, n, e_dense, e_dense / U, e_pcg, e_pcg / U, itp.cg_iterations, max(4.0 * e_pcg, n * U)))
    assert itp.cg_iterations < PCG_MAX_ITERATIONS
    assert e_dense <= max(4.0 * e_pcg, n * U)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 3. a robust graph
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_step_on_a_graph_with_robust_loop_closures():
    g = pc.graph("tl200")
    q, t, _ = util.initial_state(g, False, perturb=pc.PERTURB, seed=pc.STATE_SEED)
    base = dict(cg_early_tolerance=0.0, cg_mid_tolerance=0.0, mg_switch_iterations=0, initial_trust_region_radius=pc.RADII[0], cg_max_iterations=PCG_MAX_ITERATIONS)
    xs = []
    for opt in (dict(linear_solver=DENSE), PCG_FLOOR):
        P = capi.problem_from_graph(g, switchable=False, loop_loss=("huber", 0.1), **dict(base, **opt))
        P.solve_begin(q, t)
        P.lm_step()
        xs.append(P.linear_solution())
        _, _, _, sm = P.solve_end()
        P.close()
        assert sm.iterations[1].step_is_valid
    err = np.abs(xs[0] - xs[1]).max() / np.abs(xs[1]).max()
    print("DENSE robust tl200 huber 0.1  |x_dense - x_pcg| / |x_pcg| %.3e" % err)
    assert err <= 1e-7      # the project's figure for a converged PCG against an exact solve (test_converged_iterate_solves_the_system)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 4. trajectories against the CPU checker: linear_solver = 2, every other option at its default
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["C1", "C1F5"])
def test_first_iterations_track_the_cpu_checker(name):
    g = graphgen.config(name)
    O, P = util.oracle_problem(g, True), util.pgo_problem(g, True, linear_solver=DENSE)
    q, t, s = util.initial_state(g, True)
    _, _, _, sumo = O.solve(q, t, s)
    _, _, _, sump = P.solve(q, t, s)
    P.close()
    assert sump.num_iterations == sumo.num_iterations
    for k in range(min(sumo.num_logged, sump.num_logged)):
        a, b = sumo.iterations[k], sump.iterations[k]
        assert a.step_is_successful == b.step_is_successful
        assert abs(a.cost - b.cost) <= 1e-8 * max(a.cost, 1e-12), (k, a.cost, b.cost)
    direct_records(sump)


def test_solve_matches_the_cpu_checker_at_convergence():
    from oracle import binding as ob
    g = graphgen.config("C1")
    O, P = util.oracle_problem(g, True), util.pgo_problem(g, True, max_num_iterations=100, function_tolerance=1e-10, linear_solver=DENSE)
    q, t, s = util.initial_state(g, True)
    qo, to, so, sumo = O.solve(q, t, s, ob.default_options(max_num_iterations=100, function_tolerance=1e-10))
    qp, tp, sp, sump = P.solve(q, t, s)
    P.close()
    assert sumo.termination_type == 0 and sump.termination_type == capi.CONVERGENCE
    assert abs(sump.final_cost - sumo.final_cost) <= 1e-6 * sumo.final_cost
    dt = np.linalg.norm(tp.reshape(-1, 3) - to.reshape(-1, 3), axis=1).max()
    dr = util.rot_angle(qp.reshape(-1, 4), qo.reshape(-1, 4)).max()
    assert dt <= 1e-3 and dr <= 1e-3, (dt, dr)
    assert np.abs(sp - so).max() <= 1e-3
    direct_records(sump)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 5. determinism
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_two_solves_on_fresh_handles_give_the_same_bits():
    g = graphgen.config("C1F5")
    q, t, s = util.initial_state(g, True)
    outs = []
    for _ in range(2):
        P = util.pgo_problem(g, True, linear_solver=DENSE)
        outs.append(P.solve(q, t, s))
        P.close()
    (qa, ta, sa, ma), (qb, tb, sb, mb) = outs
    assert np.array_equal(qa, qb) and np.array_equal(ta, tb) and np.array_equal(sa, sb)
    assert ma.num_logged == mb.num_logged and ma.num_logged > 1
    assert [ma.iterations[k].cost for k in range(ma.num_logged)] == [mb.iterations[k].cost for k in range(mb.num_logged)]


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 6. a failed factorisation: an invalid step, the radius halves, the solve goes on
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_a_failed_factorisation_is_an_invalid_step_and_the_solve_goes_on():
    env = dict(os.environ, PGO_ENABLE_DEBUG_HOOKS="1")
    env.pop("PGO_DEBUG_BREAK_DENSE", None)
    out = subprocess.run([sys.executable, "-m", "tests.dense_child"], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    rec = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("DENSE ")][-1][len("DENSE "):])
    first, second = rec["steps"][1], rec["steps"][2]
    assert first["valid"] == 0 and first["successful"] == 0 and first["reason"] == capi.STEP_INVALID_FACTORIZATION and first["preconditioner"] == capi.PRECOND_DIRECT
    assert float.fromhex(second["radius"]) == 0.5 * float.fromhex(first["radius"])
    assert second["valid"] == 1 and rec["plain_first_valid"] == 1
    assert rec["termination"] == capi.CONVERGENCE
    cost, plain = float.fromhex(rec["final_cost"]), float.fromhex(rec["plain_final_cost"])
    print("DENSE invalid step: final cost %.12e, undisturbed %.12e" % (cost, plain))
    assert abs(cost - plain) <= 1e-6 * plain


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 7. contract
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def chain(n):
    return graphgen.generate(n, 0, odom_f_max=1, seed=4)


def test_more_than_the_limit_is_refused_at_solve_begin():
    g = chain(capi.DENSE_MAX_KEYFRAMES + 1)
    q, t, s = util.initial_state(g, True)
    P = util.pgo_problem(g, True, linear_solver=DENSE)
    with pytest.raises(capi.PgoError) as e:
        P.solve_begin(q, t, s)
    assert e.value.code == PGO_ERR_INVALID_ARG and b"PGO_DENSE_MAX_KEYFRAMES" in P.lib.pgo_last_error(P.h)
    with pytest.raises(capi.PgoError) as e:
        P.solve(q, t, s)
    assert e.value.code == PGO_ERR_INVALID_ARG
    P.close()


def test_the_limit_itself_runs_a_step():
    """a memory check: n = 6144, a 302 MB matrix"""
    g = chain(capi.DENSE_MAX_KEYFRAMES)
    q, t, s = util.initial_state(g, True, perturb=0.01, seed=2)
    P = util.pgo_problem(g, True, linear_solver=DENSE)
    P.solve_begin(q, t, s)
    P.lm_step()
    _, _, _, sm = P.solve_end()
    P.close()
    it = sm.iterations[1]
    print("DENSE limit: 1024 keyframes, system + factor %.2f ms, sweeps %.2f ms" % (it.seconds_system * 1e3, it.seconds_pcg * 1e3))
    assert it.step_is_valid and it.preconditioner == capi.PRECOND_DIRECT and it.cg_iterations == 0


def test_a_handle_with_a_communicator_is_refused():
    g = graphgen.config("C1")
    q, t, s = util.initial_state(g, True)
    P = util.pgo_problem(g, True, linear_solver=DENSE)
    group = capi.local_group_create(1)
    P.comm_init_local(0, 1, group)
    with pytest.raises(capi.PgoError) as e:
        P.solve_begin(q, t, s)
    assert e.value.code == PGO_ERR_STATE and b"one GPU only: a communicator is attached" in P.lib.pgo_last_error(P.h)
    P.close()
    capi.local_group_destroy(group)


def test_the_hooks_in_dense_mode():
    g = pc.graph("tl200")
    q, t, s = pc.state(g)
    P = util.pgo_problem(g, True, linear_solver=DENSE)
    P.solve_begin(q, t, s)
    with pytest.raises(capi.PgoError) as e:
        P.apply_preconditioner(capi.PRECOND_BLOCK_JACOBI, np.zeros(6 * g.n_poses))
    assert e.value.code == PGO_ERR_STATE
    with pytest.raises(capi.PgoError) as e:
        P.mg_level_parents(0)
    assert e.value.code == PGO_ERR_STATE
    # the normal operator is the block-CSR one dense mode assembles: the model's matrix
    lin = pc.linearisation("tl200")
    A, _ = pc.system("tl200", 1e4)
    v = np.zeros(6 * g.n_poses); v[lin.rows] = np.random.default_rng(0).standard_normal(len(lin.rows))
    y = P.apply_normal_operator(v)
    assert np.abs(y[lin.rows] - A @ v[lin.rows]).max() <= 1e-10 * np.abs(A @ v[lin.rows]).max()
    P.lm_step()
    assert np.isfinite(P.linear_solution()).all()
    P.solve_end()
    P.close()


def test_one_handle_switches_between_the_pcg_and_the_dense_solver():
    g = graphgen.config("C1")
    q, t, s = util.initial_state(g, True)
    P = util.pgo_problem(g, True)
    outs = []
    for solver in (capi.LINEAR_PCG_MATRIX_FREE, DENSE, capi.LINEAR_PCG_MATRIX_FREE):
        P.set_options(linear_solver=solver)
        outs.append(P.solve(q, t, s))
    P.close()
    (qa, ta, sa, ma), (_, _, _, md), (qb, tb, sb, mb) = outs
    direct_records(md)
    assert ma.cg_iterations > 0 and mb.cg_iterations == ma.cg_iterations
    assert np.array_equal(qa, qb) and np.array_equal(ta, tb) and np.array_equal(sa, sb)
    assert [ma.iterations[k].cost for k in range(ma.num_logged)] == [mb.iterations[k].cost for k in range(mb.num_logged)]
    assert abs(md.final_cost - ma.final_cost) <= 1e-6 * ma.final_cost
