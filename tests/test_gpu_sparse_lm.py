"""GPU: the exact LM step and solve of libpgo_sparse.so (pgo_sparse_lm_*; csrc/pgo_sparse_lm.hpp, sparse_cholesky.SparseLm / solve_exact).

  1. the kernels against the host instantiation (tests/native/sparse_lm_host.cpp) and the np.longdouble system;  2. the step against the dense solver of a handle, plain
  and robust;  3. solve trajectories against the CPU checker, below and above the dense limit, and against the handle's own dense solve;  4. convergence;  5. determinism;
  6. the contract: busy handles, an untouched handle, a failed factorisation.

u = 2^-53, eta and the bound eta <= n u as in tests/test_gpu_dense_cholesky.py (derived, not measured), on the FULL damped system where the switches' steps are there.
Every test prints its figures (`SPARSELM ...`) before it asserts; profiles/sparse_lm_check.txt records them."""
import numpy as np
import pytest

from solve_keyframe_pose_graph_amd import capi, graphgen
from solve_keyframe_pose_graph_amd import sparse_cholesky as sc
from tests import precond_cases as pc
from tests import sparse_lm_cases as lc
from tests import util
from tests.precond_child import linear_iterate

pytestmark = pytest.mark.gpu

U = lc.U
DENSE = capi.LINEAR_DENSE_CHOLESKY
ORDERS = (sc.ORDER_NATURAL, sc.ORDER_RCM)
GRAPHS = {
    "nine": lc.nine,
    "k11": lambda: lc.chain(11, [(9, 1)]),
    "k22": lambda: lc.chain(22, [(20, 2), (15, 4), (4, 15)], constant=(7,)),
    "tl200": lambda: lc.from_pose_graph(pc.graph("tl200")),
}


@pytest.fixture(scope="module")
def shim():
    return lc.load_shim()


class DeviceLm:
    """SparseCholesky + SparseLm of one of lc's graphs"""

    def __init__(self, graph, ordering):
        N, free, rel, sw = graph
        self.ins = lc.in_system_of(N, free, rel, sw)
        self.hi, self.lo = lc.pairs_of(self.ins, rel, sw)
        self.F = sc.SparseCholesky(N, self.ins, self.hi, self.lo, ordering)
        self.L = sc.SparseLm(self.F, free, rel[:, 0], rel[:, 1], sw[:, 0], sw[:, 1])

    def step(self, B, radius):
        return self.L.step(B.diag, B.grad, B.off, B.c, B.hss, B.gs, radius)

    def close(self):
        self.L.close(); self.F.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 1. the kernels against the host
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", pc.RADII)
@pytest.mark.parametrize("ordering", ORDERS)
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_the_kernels_against_the_host_instantiation(shim, name, ordering, radius):
    N, free, rel, sw = graph = GRAPHS[name]()
    B = lc.jacobian_blocks(11, N, rel, sw)
    H, ins, hi, lo = lc.host_lm(shim, graph, ordering)
    H.set_scale(B)
    rc, hd, hs, hout = H.step(B, radius)
    H.close()
    assert rc == 0
    D = DeviceLm(graph, ordering)
    D.L.set_scale(B.diag, B.hss)
    d, s, model, norm, ms = D.step(B, radius)
    d2, s2, model2, norm2, _ = D.step(B, radius)
    info = D.F.info()[0]
    D.close()
    F = lc.full_system(N, ins, rel, sw, B, radius)
    x, xh = F.vector(d, s), F.vector(hd, hs)
    n = len(x)
    e = lc.eta(F.H, -F.g, x)
    diff = float(np.abs(x - xh).max()) / float(np.abs(xh).max())
    want = lc.model_cost_change(F, x)
    print("SPARSELM kernels %-6s ordering %d radius %.0e  n %d  %d tiles of L  eta %.3e = %.2f u (bound n u = %.3e)  |d - d_host| / |d_host| %.3e (bound 2 n u = %.3e)  model %.12e (host %.12e, relative error to longdouble %.2e)  factor %.3f ms"
          % (name, info["ordering"], radius, n, info["l_tiles"], e, e / U, n * U, diff, 2 * n * U, model, hout[0], abs(model - want) / abs(want), ms))
    assert e <= n * U
    assert diff <= 2 * n * U
    assert abs(model - want) <= 1e-12 * abs(want) and abs(norm - hout[1]) <= 1e-13 * hout[1]
    assert not d.reshape(-1)[np.repeat(ins == 0, 6)].any()
    assert np.array_equal(d, d2) and np.array_equal(s, s2) and model == model2 and norm == norm2      # no atomics, fixed summation order: the same bits


def test_a_failed_pivot_is_reported_and_the_next_step_is_that_of_a_fresh_object():
    N, free, rel, sw = graph = GRAPHS["k22"]()
    B = lc.jacobian_blocks(5, N, rel, sw)
    D = DeviceLm(graph, sc.ORDER_RCM)
    with pytest.raises(capi.PgoError) as e:
        D.step(B, 1e4)
    assert e.value.code == sc.ERR_STATE      # no scale yet
    D.L.set_scale(B.diag, B.hss)
    bad = B.diag.copy(); bad[12] -= 200.0 * np.eye(6)
    with pytest.raises(capi.PgoError) as e:
        D.L.step(bad, B.grad, B.off, B.c, B.hss, B.gs, 1e4)
    assert e.value.code == sc.ERR_NUMERIC
    with pytest.raises(capi.PgoError) as e:
        D.L.step(B.diag, B.grad, B.off, B.c, -B.hss, B.gs, 1e4)      # a damped switch pivot that is not > 0
    assert e.value.code == sc.ERR_NUMERIC
    after = D.step(B, 1e4)
    D.close()
    G = DeviceLm(graph, sc.ORDER_RCM)
    G.L.set_scale(B.diag, B.hss)
    fresh = G.step(B, 1e4)
    G.close()
    assert np.array_equal(after[0], fresh[0]) and np.array_equal(after[1], fresh[1]) and after[2:4] == fresh[2:4]


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 2. the step against the dense solver
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def edges_of(g, switchable=True, constant=()):
    return sc.Edges.from_graph(g, switchable, constant)


def handle_blocks(P, q, t, s):
    """the normal blocks of a handle's first linearisation, through the hooks, after solve_begin"""
    P.solve_begin(q, t, s)
    diag, grad, off, c, hss, gs = P.normal_blocks()
    P.solve_end()
    return lc.Blocks(diag, grad, off, c, hss, gs)


def sparse_step_of_handle(P, g, switchable, constant, q, t, s, radius, ordering=sc.ORDER_AUTO):
    """-> (delta_pose [6 N], graph tuple, keyframes of the system, blocks)"""
    B = handle_blocks(P, q, t, s)
    ed = edges_of(g, switchable, constant)
    graph = (g.n_poses, None, np.stack([ed.rel_c1, ed.rel_c2], axis=1), np.stack([ed.sw_c1, ed.sw_c2], axis=1).reshape(-1, 2))
    free = np.ones(g.n_poses, np.uint8); free[list(constant)] = 0
    ref = np.zeros(g.n_poses, bool)
    for a in (ed.rel_c1, ed.rel_c2, ed.sw_c1, ed.sw_c2, ed.reg_node):
        ref[np.asarray(a, dtype=np.int64)] = True
    ins = ((free != 0) & ref).astype(np.uint8)
    hi, lo = lc.pairs_of(ins, graph[2], graph[3])
    F = sc.SparseCholesky(g.n_poses, ins, hi, lo, ordering)
    L = sc.SparseLm(F, free, ed.rel_c1, ed.rel_c2, ed.sw_c1, ed.sw_c2)
    L.set_scale(B.diag, B.hss)
    d, ds, model, norm, ms = L.step(B.diag, B.grad, B.off, B.c, B.hss, B.gs, radius)
    L.close(); F.close()
    return d.reshape(-1), ds, (g.n_poses, free, graph[2], graph[3]), ins, B


STEP_CASES = [("tl200", (), 0), ("tl600", pc.CONSTANT_TL600, 0)]


@pytest.mark.parametrize("radius", pc.RADII)
@pytest.mark.parametrize("name,constant,drop_last", STEP_CASES)
def test_the_step_equals_the_dense_solvers_to_rounding(name, constant, drop_last, radius):
    lin = pc.linearisation(name, constant, drop_last)
    A, b = pc.system(name, radius, constant, drop_last)
    n = A.shape[0]
    xd, it, P = linear_iterate(name, 1, radius, constant, drop_last, linear_solver=DENSE)
    P.close()
    assert it.step_is_valid and it.preconditioner == capi.PRECOND_DIRECT
    g = pc.graph(name, drop_last)
    q, t, s = pc.state(g)
    P = util.pgo_problem(g, True, initial_trust_region_radius=radius)      # the default, matrix-free handle
    if constant:
        P.set_nodes_constant(list(constant))
    x, _, _, _, _ = sparse_step_of_handle(P, g, True, constant, q, t, s, radius)
    P.close()
    e_sparse, e_dense = lc.eta(A, b, x[lin.rows]), lc.eta(A, b, xd[lin.rows])
    outside = np.ones(len(x), bool); outside[lin.rows] = False
    print("SPARSELM step %s constant %d radius %.0e  n %d  eta_sparse %.3e = %.2f u  eta_dense %.3e = %.2f u  bound max(4 eta_dense, n u) = %.3e  |x - x_dense| / |x_dense| %.3e"
          % (name, len(constant), radius, n, e_sparse, e_sparse / U, e_dense, e_dense / U, max(4.0 * e_dense, n * U), np.abs(x - xd).max() / np.abs(xd).max()))
    assert np.all(x[outside] == 0.0)
    assert e_sparse <= max(4.0 * e_dense, n * U)


@pytest.mark.parametrize("switchable", [False, True])
def test_the_step_on_a_graph_with_robust_loop_closures(switchable):
    """the system: the np.longdouble reduction of the handle's own (corrected) normal blocks — the oracle's model has no robust switchable edge"""
    g = pc.graph("tl200")
    radius = pc.RADII[0]
    q, t, s = util.initial_state(g, switchable, perturb=pc.PERTURB, seed=pc.STATE_SEED)
    P = capi.problem_from_graph(g, switchable=switchable, loop_loss=("huber", 0.1), initial_trust_region_radius=radius)
    x, ds, graph, ins, B = sparse_step_of_handle(P, g, switchable, (), q, t, s if switchable else None, radius)
    P.close()
    P = capi.problem_from_graph(g, switchable=switchable, loop_loss=("huber", 0.1), initial_trust_region_radius=radius, linear_solver=DENSE)
    P.solve_begin(q, t, s if switchable else None)
    P.lm_step()
    xd = P.linear_solution()
    _, _, _, sm = P.solve_end()
    P.close()
    assert sm.iterations[1].step_is_valid
    F = lc.full_system(graph[0], ins, graph[2], graph[3], B, radius)
    S, rhs, _, _, _, _ = lc.reduced(F)
    n = len(rhs)
    e_sparse, e_dense = lc.eta(S, rhs, x[F.rows]), lc.eta(S, rhs, xd[F.rows])
    e_full = lc.eta(F.H, -F.g, F.vector(x, ds))
    print("SPARSELM robust tl200 huber 0.1 switchable %d  n %d  eta_sparse %.3e = %.2f u  eta_dense %.3e = %.2f u  bound max(4 eta_dense, n u) = %.3e  full system eta %.2f u"
          % (switchable, n, e_sparse, e_sparse / U, e_dense, e_dense / U, max(4.0 * e_dense, n * U), e_full / U))
    assert e_sparse <= max(4.0 * e_dense, n * U)
    assert e_full <= len(F.g) * U


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 3. trajectories against the CPU checker
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def big_graph():
    return graphgen.generate(1100, 110, odom_f_max=5, seed=7)      # tests/test_gpu_sparse_cholesky.py's graph above the dense limit


# name -> (graph, perturbation of the start, its seed).  The checker's log of the default start has no rejected step (its one unsuccessful record is the step a tolerance
# ended the solve on); from C1F5 perturbed by 1.0 (seed 2) it accepts three steps, rejects two in a row — the radius shrinks by 2, then by 4 — and accepts the rest:
# found on the CPU with the checker alone, and asserted below.  The checker's 1 100-keyframe solve takes 0.2 s on a CPU: no cap on max_num_iterations.
TRAJECTORIES = {"C1": (lambda: graphgen.config("C1"), 0.0, 0), "C1F5": (lambda: graphgen.config("C1F5"), 0.0, 0), "C1F5_rejections": (lambda: graphgen.config("C1F5"), 1.0, 2),
                "g1100": (big_graph, 0.0, 0)}


def same_trajectory(what, sumo, sump):
    assert sump.num_iterations == sumo.num_iterations, (what, sump.num_iterations, sumo.num_iterations)
    worst = 0.0
    for k in range(min(sumo.num_logged, sump.num_logged)):
        a, b = sumo.iterations[k], sump.iterations[k]
        worst = max(worst, abs(a.cost - b.cost) / max(a.cost, 1e-12))
        assert a.step_is_successful == b.step_is_successful, (what, k)
        assert abs(a.cost - b.cost) <= 1e-8 * max(a.cost, 1e-12), (what, k, a.cost, b.cost)
    return worst


def direct_records(sm):
    for k in range(1, sm.num_logged):
        it = sm.iterations[k]
        assert it.cg_iterations == 0 and it.cg_iterations_multigrid == 0 and it.single_reduction == 0 and it.cg_residual == 0.0 and it.preconditioner == capi.PRECOND_DIRECT, k
    assert sm.cg_iterations == 0 and sm.pcg_retries == 0


@pytest.mark.parametrize("name", sorted(TRAJECTORIES))
def test_the_solve_tracks_the_cpu_checker(name):
    make, perturb, seed = TRAJECTORIES[name]
    g = make()
    q, t, s = util.initial_state(g, True, perturb=perturb, seed=seed)
    _, _, _, sumo = util.oracle_problem(g, True).solve(q, t, s)
    if name == "C1F5_rejections":      # rejected steps in the checker's own log, with accepted ones on both sides
        assert [sumo.iterations[k].step_is_successful for k in range(6)] == [1, 1, 1, 0, 0, 1] and all(sumo.iterations[k].step_is_valid for k in range(6))
    P = util.pgo_problem(g, True)      # a DEFAULT handle: matrix-free
    tm = {}
    qs, ts, ss, sums = sc.solve_exact(P, edges_of(g), q, t, s, timings=tm)
    worst = same_trajectory(name, sumo, sums)
    direct_records(sums)
    line = "SPARSELM trajectory %-5s %d keyframes  %d iterations (%d unsuccessful)  worst relative cost difference to the checker %.3e  final cost %.9e  %d tiles of L, last factor %.3f ms" % (
        name, g.n_poses, sums.num_iterations, sums.num_unsuccessful_steps, worst, sums.final_cost, tm["info"]["l_tiles"], tm["factor_ms"])
    if g.n_poses <= capi.DENSE_MAX_KEYFRAMES:
        P.set_options(linear_solver=DENSE)
        _, _, _, sumd = P.solve(q, t, s)
        line += "  against the handle's dense solve %.3e" % same_trajectory(name + " dense", sumd, sums)
    P.close()
    print(line)
    assert sums.termination_type == sumo.termination_type


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 4. convergence
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_solve_matches_the_cpu_checker_at_convergence():
    from oracle import binding as ob
    g = graphgen.config("C1")
    q, t, s = util.initial_state(g, True)
    qo, to, so, sumo = util.oracle_problem(g, True).solve(q, t, s, ob.default_options(max_num_iterations=100, function_tolerance=1e-10))
    P = util.pgo_problem(g, True)
    qp, tp, sp, sump = sc.solve_exact(P, edges_of(g), q, t, s, max_num_iterations=100, function_tolerance=1e-10)
    P.close()
    dt = np.linalg.norm(tp.reshape(-1, 3) - to.reshape(-1, 3), axis=1).max()
    dr = util.rot_angle(qp.reshape(-1, 4), qo.reshape(-1, 4)).max()
    print("SPARSELM convergence C1: %d iterations (checker %d)  final cost %.12e (checker %.12e)  max |dt| %.3e  max rotation %.3e  max |ds| %.3e"
          % (sump.num_iterations, sumo.num_iterations, sump.final_cost, sumo.final_cost, dt, dr, np.abs(sp - so).max()))
    assert sumo.termination_type == 0 and sump.termination_type == capi.CONVERGENCE
    assert abs(sump.final_cost - sumo.final_cost) <= 1e-6 * sumo.final_cost
    assert dt <= 1e-3 and dr <= 1e-3
    assert np.abs(sp - so).max() <= 1e-3
    direct_records(sump)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 5. determinism
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_two_solves_on_fresh_objects_give_the_same_bits():
    g = graphgen.config("C1F5")
    q, t, s = util.initial_state(g, True)
    outs = []
    for _ in range(2):
        P = util.pgo_problem(g, True)
        outs.append(sc.solve_exact(P, edges_of(g), q, t, s))
        P.close()
    (qa, ta, sa, ma), (qb, tb, sb, mb) = outs
    assert np.array_equal(qa, qb) and np.array_equal(ta, tb) and np.array_equal(sa, sb)
    assert ma.num_logged == mb.num_logged and ma.num_logged > 1
    assert [ma.iterations[k].cost for k in range(ma.num_logged)] == [mb.iterations[k].cost for k in range(mb.num_logged)]


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 6. the contract
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_a_handle_inside_a_solve_or_with_a_communicator_is_refused():
    g = graphgen.config("C1")
    q, t, s = util.initial_state(g, True)
    P = util.pgo_problem(g, True)
    P.solve_begin(q, t, s)
    with pytest.raises(capi.PgoError) as e:
        sc.solve_exact(P, edges_of(g), q, t, s)
    assert e.value.code == sc.ERR_STATE
    P.lm_step()      # ... and the open solve is still the handle's
    _, _, _, sm = P.solve_end()
    assert sm.num_logged == 2
    P.close()
    P = util.pgo_problem(g, True)
    group = capi.local_group_create(1)
    P.comm_init_local(0, 1, group)
    with pytest.raises(capi.PgoError) as e:
        sc.solve_exact(P, edges_of(g), q, t, s)
    assert e.value.code == sc.ERR_STATE and "communicator" in str(e.value)
    P.close()
    capi.local_group_destroy(group)


def test_the_handle_is_untouched_by_an_exact_solve():
    g = graphgen.config("C1")
    q, t, s = util.initial_state(g, True)
    P = util.pgo_problem(g, True)
    fresh = P.solve(q, t, s)
    P.close()
    P = util.pgo_problem(g, True)
    sc.solve_exact(P, edges_of(g), q, t, s)
    after = P.solve(q, t, s)
    P.close()
    for a, b in zip(fresh[:3], after[:3]):
        assert np.array_equal(a, b)
    assert [fresh[3].iterations[k].cost for k in range(fresh[3].num_logged)] == [after[3].iterations[k].cost for k in range(after[3].num_logged)]
    assert fresh[3].cg_iterations == after[3].cg_iterations


def test_a_failed_factorisation_is_an_invalid_step_and_the_solve_goes_on():
    """the second linearisation's diagonal block of keyframe 50 is made indefinite through the wrapped normal_blocks callback, once: the point is linearised again
    after the invalid step, so the disturbance lasts one iteration"""
    g = graphgen.config("C1")
    q, t, s = util.initial_state(g, True)
    opt = dict(max_num_iterations=100, function_tolerance=1e-10)
    P = util.pgo_problem(g, True)
    _, _, _, plain = sc.solve_exact(P, edges_of(g), q, t, s, **opt)
    seen = []

    def disturb(call, diag, grad, off, c, hss, gs):
        seen.append(call)
        if call == 1:
            diag[50] -= 1e6 * np.eye(6)

    _, _, _, sm = sc.solve_exact(P, edges_of(g), q, t, s, hooks={"normal_blocks": disturb}, **opt)
    P.close()
    first, second = sm.iterations[2], sm.iterations[3]
    print("SPARSELM invalid step: final cost %.12e, undisturbed %.12e; %d iterations, undisturbed %d" % (sm.final_cost, plain.final_cost, sm.num_iterations, plain.num_iterations))
    assert plain.iterations[1].step_is_successful == 1 and sm.iterations[1].cost == plain.iterations[1].cost
    assert first.step_is_valid == 0 and first.step_is_successful == 0 and first.reason == capi.STEP_INVALID_FACTORIZATION and first.preconditioner == capi.PRECOND_DIRECT
    assert second.trust_region_radius == 0.5 * first.trust_region_radius and second.step_is_valid == 1
    assert seen[:3] == [0, 1, 2] and sm.num_unsuccessful_steps >= 1
    assert sm.termination_type == capi.CONVERGENCE and plain.termination_type == capi.CONVERGENCE
    assert abs(sm.final_cost - plain.final_cost) <= 1e-6 * plain.final_cost
