"""GPU: Huber and Cauchy robust losses on relative-pose edges (pgo_add_relpose_edges_robust: ceres::HuberLoss / ceres::CauchyLoss with Ceres' Corrector on the SixDOFError loop
edge, reference src/PoseGraphSLAM.cpp:793-796 with :401-402) through every layer: K1's LOSS instantiations (cost-only included), K2, both matvec forms, the two-level method, the
multigrid, two ranks, the C-ABI contract.

The yardstick is the REWEIGHTED ORACLE PROBLEM AT x: at a given point the linearisation of a robust edge is exactly that of the plain edge of weight w_e c_e(x), c_e = sqrt(rho'(s_e)),
s_e = |r_e|^2 — so the checker is the oracle's plain problem with the loop weights w_e c_e(x), c_e computed in numpy from the oracle's own residuals (ob.eval_relpose).  Only the cost
(0.5 rho(s), not 0.5 |c r|^2) is formed here from the same s.

Fixture: small_graph(300, 40, f=2, seed=11, outlier_frac=0.2) — 597 odometry edges + 40 loops (8 outliers) = 637 relative-pose edges: nine full 64-lane K1 tiles and a partial one, robust
and plain lanes mixed inside a tile; at the initial state the inlier loops reach |r| = 0.53 and the outliers 2.0-4.9 (nearly every loop beyond Huber(0.1)'s branch point; with the odometry edges under the loss 67 edges lie
beyond it and 570 inside), at the solution 11 loops lie beyond and 29 inside."""
import numpy as np
import pytest

from oracle import binding as ob
from solve_keyframe_pose_graph_amd import capi, graphgen, sharding
from tests import util

pytestmark = pytest.mark.gpu

HUBER, CAUCHY = ("huber", 0.1), ("cauchy", 1.0)      # the reference's robust_norm and its commented alternative (src/PoseGraphSLAM.cpp:401-402)


def rho_c(loss, s):
    """rho(s) and c = sqrt(rho'(s)) in numpy; loss None: the trivial loss"""
    s = np.asarray(s, dtype=np.float64)
    if loss is None:
        return s.copy(), np.ones_like(s)
    kind, a = loss
    b = a * a
    if kind == "huber":
        root = np.sqrt(np.maximum(s, b))
        return np.where(s > b, 2.0 * a * root - b, s), np.where(s > b, np.sqrt(a / root), 1.0)
    u = 1.0 + s / b
    return b * np.log(u), np.sqrt(1.0 / u)


class Edges:
    """the relative-pose edges of a graph in one add order, each with its loss (None: plain)"""

    def __init__(self, g, loop_loss, odom_loss=None, loops_first=False, loop_mask=None):
        il = np.arange(g.n_loops) if loop_mask is None else np.flatnonzero(loop_mask)
        odom = (g.odom_c1, g.odom_c2, g.odom_T, g.odom_w, odom_loss)
        loops = (g.loop_c1[il], g.loop_c2[il], g.loop_T[il], g.loop_w[il], loop_loss)
        self.groups = [loops, odom] if loops_first else [odom, loops]
        self.c1, self.c2, self.T, self.w = (np.concatenate([grp[k] for grp in self.groups]) for k in range(4))
        self.loss = [grp[4] for grp in self.groups for _ in range(len(grp[0]))]
        self.is_loop = np.concatenate([np.full(len(grp[0]), grp is loops) for grp in self.groups])
        self.g = g

    def problem(self, **opt):
        P = capi.Problem(**opt)
        for c1, c2, T, w, loss in self.groups:
            P.add_relpose_edges(c1, c2, T, w, loss=loss)
        if len(self.g.reg_node):
            P.set_node_regularizers(self.g.reg_node, self.g.reg_T, self.g.reg_w)
        return P

    def at(self, q, t):
        """(s_e, rho_e, c_e) of every edge at (q, t), from the oracle's residuals at the edges' own weights"""
        q = np.asarray(q).reshape(-1, 4); t = np.asarray(t).reshape(-1, 3)
        s = np.array([np.sum(ob.eval_relpose(q[a], t[a], q[b], t[b], self.T[e], self.w[e])[0] ** 2) for e, (a, b) in enumerate(zip(self.c1, self.c2))])
        rho, c = np.empty_like(s), np.empty_like(s)
        for loss in set(self.loss):
            m = np.array([x == loss for x in self.loss])
            rho[m], c[m] = rho_c(loss, s[m])
        return s, rho, c

    def reweighted_oracle(self, c):
        O = ob.OracleProblem()
        O.add_relpose_edges(self.c1, self.c2, self.T, self.w * c)
        if len(self.g.reg_node):
            O.set_node_regularizers(self.g.reg_node, self.g.reg_T, self.g.reg_w)
        return O

    def robust_cost(self, q, t):
        """0.5 (sum over plain blocks |r|^2 + sum over robust blocks rho) through the oracle at (q, t)"""
        s, rho, c = self.at(q, t)
        _, res, _ = self.reweighted_oracle(c).evaluate(q, t, np.zeros(0), want_gradient=False)
        return 0.5 * (rho.sum() + np.sum(res[6 * len(s):] ** 2))


@pytest.fixture(scope="module")
def fixture_graph():
    g = util.small_graph(300, 40, f=2, seed=11, outlier_frac=0.2)
    assert g.n_odom == 597 and g.n_loops == 40 and int(np.sum(g.loop_is_outlier != 0)) == 8
    return g


@pytest.fixture(scope="module")
def perturbed(fixture_graph):
    q, t, _ = util.initial_state(fixture_graph, False, perturb=0.01, seed=3)
    return q, t


# ---- 1. evaluate
@pytest.mark.parametrize("case", ["huber-loops", "cauchy-loops", "huber-all", "huber-loops-first"])
def test_evaluate_is_ceres_evaluate_with_the_loss_applied(fixture_graph, perturbed, case):
    g = fixture_graph
    E = {"huber-loops": lambda: Edges(g, HUBER), "cauchy-loops": lambda: Edges(g, CAUCHY), "huber-all": lambda: Edges(g, HUBER, odom_loss=HUBER),
         "huber-loops-first": lambda: Edges(g, HUBER, loops_first=True)}[case]()      # (the last: the loss plane follows the edges, not their position)
    q, t = perturbed
    s, rho, c = E.at(q, t)
    robust = np.array([x is not None for x in E.loss])
    if case.startswith("huber"):
        assert np.sum(s[robust] > 0.01) >= 5                                          # the fixture guarantees edges beyond a ...
    if case == "huber-all":
        assert np.sum(s[robust] < 0.01) >= 5                                          # ... and, with the odometry edges under the loss, both branches (67 and 570)
    O = E.reweighted_oracle(c)
    co, ro, go = O.evaluate(q, t, np.zeros(0))
    want_cost = 0.5 * (rho.sum() + np.sum(ro[6 * len(s):] ** 2))
    wrong_cost = co                                                                  # 0.5 sum rho' s: what an implementation summing |c r|^2 reports
    assert abs(wrong_cost - want_cost) > 1e-6 * want_cost                            # ... and the bound below tells the two apart
    P = E.problem()
    cp, rp, gp = P.evaluate(q, t)
    P.close()
    print("cost %.15e want %.15e (sum rho' s: %.15e)  residuals %.3e  gradient %.3e" % (cp, want_cost, wrong_cost, np.abs(rp - ro).max(), np.abs(gp - go).max()))
    assert abs(cp - want_cost) <= 1e-12 * max(1.0, abs(want_cost))
    assert np.abs(rp - ro).max() <= 1e-12 * max(1.0, np.abs(ro).max())
    assert np.abs(gp - go).max() <= 1e-11 * max(1.0, np.abs(go).max())


# ---- 2. blocks
def test_jacobian_and_normal_blocks_are_the_reweighted_oracles(fixture_graph, perturbed):
    g = fixture_graph
    E = Edges(g, HUBER)
    q, t = perturbed
    _, _, c = E.at(q, t)
    O = E.reweighted_oracle(c)
    P = E.problem()
    P.evaluate(q, t)
    none = np.zeros(0)
    J1o, J2o, _ = O.jacobian_blocks(q, t, none, 0)
    J1p, J2p, _ = P.jacobian_blocks(0)
    scale = max(1.0, np.abs(J1o).max())
    assert np.abs(J1p - J1o).max() <= 1e-12 * scale and np.abs(J2p - J2o).max() <= 1e-12 * scale
    N = g.n_poses
    H = O.dense_normal_matrix(q, t, none)
    _, _, go = O.evaluate(q, t, none)
    diag, grad, off, _, _, _ = P.normal_blocks()
    P.close()
    tol = 1e-11 * max(1.0, np.abs(H).max())
    for n in range(N):
        assert np.abs(diag[n] - H[6 * n:6 * n + 6, 6 * n:6 * n + 6]).max() <= tol
    assert np.abs(grad.reshape(-1) - go[:6 * N]).max() <= 1e-11 * max(1.0, np.abs(go).max())
    acc = {}      # the oracle's dense matrix holds the SUM over parallel edges
    for e in range(len(E.c1)):
        acc.setdefault((E.c1[e], E.c2[e]), np.zeros((6, 6)))
        acc[(E.c1[e], E.c2[e])] += off[e]
    for (a, b), blk in acc.items():
        if (b, a) in acc:
            blk = blk + acc[(b, a)].T
        assert np.abs(blk - H[6 * a:6 * a + 6, 6 * b:6 * b + 6]).max() <= tol


# ---- 3. operator
@pytest.mark.parametrize("linear_solver", [0, 1])
def test_normal_operator_with_robust_and_switchable_loops_is_the_schur_complement(linear_solver):
    """(H_reduced + damping) x on the device, both matvec forms, with half of the loops Huber relative-pose edges and the other half switchable, against the dense Schur
    complement of the reweighted oracle's H — built exactly as tests/test_gpu_parity.py::test_normal_operator_is_schur_complement builds it."""
    g = util.small_graph(260, 60, f=5, seed=2, outlier_frac=0.2)
    robust = np.arange(g.n_loops) % 2 == 0
    isw = np.flatnonzero(~robust)
    q, t, _ = util.initial_state(g, False, perturb=0.02, seed=6)
    s = np.full(len(isw), 0.99) + np.random.default_rng(6).normal(size=len(isw)) * 0.02
    E = Edges(g, HUBER, loop_mask=robust)
    sq, _, c = E.at(q, t)
    assert np.sum(sq[E.is_loop] > 0.01) >= 5      # robust loops beyond a: their weights really are w c, c < 1
    O = E.reweighted_oracle(c)
    O.add_switchable_edges(g.loop_c1[isw], g.loop_c2[isw], g.loop_T[isw], g.loop_w[isw], np.arange(len(isw)))
    P = E.problem(linear_solver=linear_solver)
    P.add_switchable_edges(g.loop_c1[isw], g.loop_c2[isw], g.loop_T[isw], g.loop_w[isw], np.arange(len(isw), dtype=np.int32))
    N = g.n_poses
    H = O.dense_normal_matrix(q, t, s)
    P.solve_begin(q, t, s)
    radius = 1e4
    scale = 1.0 / (1.0 + np.sqrt(np.diag(H)))
    D2 = np.clip(scale ** 2 * np.diag(H), 1e-6, 1e32) / radius
    lam = D2 / scale ** 2
    Hd = H + np.diag(lam)
    A = Hd[:6 * N, :6 * N] - Hd[:6 * N, 6 * N:] @ np.linalg.solve(Hd[6 * N:, 6 * N:], Hd[6 * N:, :6 * N])
    x = np.random.default_rng(0).normal(size=6 * N)
    y = P.apply_normal_operator(x)
    P.solve_end()
    P.close()
    assert np.abs(y - A @ x).max() <= 1e-10 * np.abs(A @ x).max()


# ---- 4. a huge Huber parameter is the plain path
def test_huber_that_never_leaves_its_quadratic_branch_is_the_plain_solve(fixture_graph, perturbed):
    g = fixture_graph
    huge = ("huber", 1e30)
    E = Edges(g, huge, odom_loss=huge)
    q, t = perturbed
    R, Q = E.problem(), util.pgo_problem(g, False)
    (cr, rr, gr), (cq, rq, gq) = R.evaluate(q, t), Q.evaluate(q, t)
    rel = lambda x, y: np.abs(np.asarray(x) - np.asarray(y)).max() <= 1e-13 * max(1.0, np.abs(y).max())      # (no bit equality demanded: the summation order may differ)
    assert abs(cr - cq) <= 1e-13 * cq and rel(rr, rq) and rel(gr, gq)
    q0, t0, _ = util.initial_state(g, False)
    qr, tr, _, sr = R.solve(q0, t0)
    qq, tq, _, sq = Q.solve(q0, t0)
    R.close(); Q.close()
    assert sr.num_iterations == sq.num_iterations and sr.num_logged == sq.num_logged and sq.num_iterations >= 3      # (the default budget: 10 iterations)
    for k in range(sq.num_logged):
        assert sr.iterations[k].step_is_successful == sq.iterations[k].step_is_successful
        assert abs(sr.iterations[k].cost - sq.iterations[k].cost) <= 1e-13 * sq.iterations[k].cost, k
    assert rel(qr, qq) and rel(tr, tq)


# ---- 5. the solve stops at a stationary point of the robust objective
STATIONARY = dict(cg_rel_tolerance=1e-12, max_num_iterations=200, function_tolerance=0.0, parameter_tolerance=0.0)
_tolerance = {}


def gradient_tolerance(g, loss):
    """1e-6 x the max-norm of the initial gradient of the robust objective, taken from evaluate"""
    if loss not in _tolerance:
        q, t, _ = util.initial_state(g, False)
        P = Edges(g, loss).problem()
        _, _, grad = P.evaluate(q, t)
        P.close()
        _tolerance[loss] = 1e-6 * np.abs(grad).max()
    return _tolerance[loss]


@pytest.mark.parametrize("linear_solver", [0, 1])
@pytest.mark.parametrize("loss", [HUBER, CAUCHY])
def test_solve_converges_to_a_stationary_point_of_the_robust_objective(fixture_graph, loss, linear_solver):
    g = fixture_graph
    E = Edges(g, loss)
    tol = gradient_tolerance(g, loss)
    q, t, _ = util.initial_state(g, False)
    P = E.problem(linear_solver=linear_solver, gradient_tolerance=tol, **STATIONARY)
    qs, ts, _, summ = P.solve(q, t)
    P.close()
    s, rho, c = E.at(qs, ts)
    _, res, grad = E.reweighted_oracle(c).evaluate(qs, ts, np.zeros(0))
    want_cost = 0.5 * (rho.sum() + np.sum(res[6 * len(s):] ** 2))
    costs = [summ.iterations[k].cost for k in range(summ.num_logged)]
    print("%s solver %d: %d iterations, termination %d, |g| %.3e (tolerance %.3e), final cost %.15e want %.15e; loops beyond / inside a^2: %d / %d" % (
        loss, linear_solver, summ.num_iterations, summ.termination_type, np.abs(grad).max(), tol, summ.final_cost, want_cost,
        np.sum(s[E.is_loop] > loss[1] ** 2), np.sum(s[E.is_loop] < loss[1] ** 2)))
    assert summ.termination_type == capi.CONVERGENCE, summ.message
    assert np.abs(grad).max() <= 2 * tol
    assert abs(summ.final_cost - want_cost) <= 1e-10 * want_cost
    for k in range(1, summ.num_logged):
        if summ.iterations[k].step_is_successful:
            assert costs[k] < costs[k - 1], (k, costs[k - 1], costs[k])
    if loss == HUBER:      # both branches of the loss at the solution (a CPU probe of the IRLS fixed point gave 11 and 29)
        assert np.sum(s[E.is_loop] > loss[1] ** 2) >= 5 and np.sum(s[E.is_loop] < loss[1] ** 2) >= 5


@pytest.mark.parametrize("linear_solver", [0, 1])
def test_plain_solve_reaches_the_same_gradient_bound(fixture_graph, linear_solver):
    """The same graph with plain loops under the same options (the Huber run's gradient tolerance included): the bound the robust solves are held to is reachable by the existing path."""
    g = fixture_graph
    E = Edges(g, None)
    tol = gradient_tolerance(g, HUBER)
    q, t, _ = util.initial_state(g, False)
    P = E.problem(linear_solver=linear_solver, gradient_tolerance=tol, **STATIONARY)
    qs, ts, _, summ = P.solve(q, t)
    P.close()
    _, _, grad = E.reweighted_oracle(np.ones(len(E.c1))).evaluate(qs, ts, np.zeros(0))
    print("plain solver %d: %d iterations, |g| %.3e (tolerance %.3e)" % (linear_solver, summ.num_iterations, np.abs(grad).max(), tol))
    assert summ.termination_type == capi.CONVERGENCE, summ.message
    assert np.abs(grad).max() <= 2 * tol


# ---- 6. the multigrid consumes K1's corrected blocks
def test_multigrid_solve_follows_the_block_jacobi_solve():
    g = graphgen.generate(6000, 600, odom_f_max=2, seed=7, outlier_frac=0.1)
    q, t, _ = util.initial_state(g, False)
    opts = dict(mg_switch_iterations=0, cg_rel_tolerance=1e-12, max_num_iterations=6)
    M = capi.problem_from_graph(g, switchable=False, loop_loss=HUBER, **opts)
    _, _, _, sm = M.solve(q, t)
    M.close()
    B = capi.problem_from_graph(g, switchable=False, loop_loss=HUBER, mg_min_keyframes=0, mg_min_keyframes_switchable=0, coarse_aggregates=0, **opts)
    _, _, _, sb = B.solve(q, t)
    B.close()
    assert any((sm.iterations[k].preconditioner & 15) == capi.PRECOND_MULTIGRID for k in range(sm.num_logged))
    assert all((sb.iterations[k].preconditioner & 15) == capi.PRECOND_BLOCK_JACOBI for k in range(sb.num_logged))
    assert sm.num_logged == sb.num_logged
    for k in range(sb.num_logged):
        assert abs(sm.iterations[k].cost - sb.iterations[k].cost) <= 1e-8 * sb.iterations[k].cost, (k, sm.iterations[k].cost, sb.iterations[k].cost)


# ---- 7. two in-process ranks
def test_two_ranks_reproduce_the_single_handle(fixture_graph):
    import threading
    from tests.test_gpu_two_ranks_one_gpu import InProcessAllReduce
    g = fixture_graph
    q, t, _ = util.initial_state(g, False)
    opts = dict(cg_rel_tolerance=1e-12, cg_max_iterations=20000)
    P = capi.problem_from_graph(g, switchable=False, loop_loss=HUBER, **opts)
    q1, t1, _, sum1 = P.solve(q, t)
    c_ref, _, g_ref = P.evaluate(q, t)
    P.close()
    world = 2
    parts = sharding.partition(g, world, "chain")
    ar = InProcessAllReduce(world, "local")
    out, grads, err = [None] * world, [None] * world, []

    def run(rank):
        try:
            Pr = capi.problem_from_graph(g, switchable=False, loop_loss=HUBER, edge_slice=parts[rank], **opts)
            ar.attach(Pr, rank)
            c, _, gr = Pr.evaluate(q, t)
            grads[rank] = (c, gr)
            out[rank] = Pr.solve(q, t)
            Pr.comm_destroy()
            Pr.close()
        except Exception as e:   # make a failing rank release the other
            err.append(e)
            ar.barrier.abort()
    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for x in th:
        x.start()
    for x in th:
        x.join(timeout=600)
    assert not err, err
    ar.close()
    for r in range(world):
        c, gr = grads[r]
        assert abs(c - c_ref) <= 1e-12 * c_ref
        assert np.abs(gr - g_ref).max() <= 1e-10 * np.abs(g_ref).max()
        qr, tr, _, sumr = out[r]
        assert sumr.num_iterations == sum1.num_iterations
        assert abs(sumr.final_cost - sum1.final_cost) <= 1e-9 * sum1.final_cost
        assert np.abs(tr - t1).max() <= 1e-7
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


# ---- 8. contract
def test_invalid_loss_arguments_add_nothing():
    P = capi.Problem()
    T = np.eye(4).flatten(order="F").reshape(1, 16)
    P.add_relpose_edges([1], [0], T, [1.0])
    for bad in [(3, 0.1), (-1, 0.1), ("huber", 0.0), ("huber", -0.1), ("cauchy", float("nan")), ("cauchy", float("inf")), ("huber", float("-inf"))]:
        with pytest.raises(capi.PgoError) as e:
            P.add_relpose_edges([2], [1], T, [1.0], loss=bad)
        assert e.value.code == -1      # PGO_ERR_INVALID_ARG
        assert P.num_relpose_edges() == 1
    P.add_relpose_edges([2], [1], T, [1.0], loss=("trivial", -5.0))      # PGO_LOSS_TRIVIAL is pgo_add_relpose_edges: its parameter is not looked at
    assert P.num_relpose_edges() == 2
    kind, a = P.relpose_edge_loss()
    assert list(kind) == [0, 0] and list(a) == [0.0, 0.0]
    P.close()


def test_edge_losses_round_trip_over_plain_robust_and_vio_edges():
    g = util.small_graph(40, 4, f=2, seed=5)
    P = capi.Problem()
    add = lambda lo, hi, loss: P.add_relpose_edges(g.odom_c1[lo:hi], g.odom_c2[lo:hi], g.odom_T[lo:hi], g.odom_w[lo:hi], loss=loss)
    add(0, 3, None)
    add(3, 5, ("huber", 0.1))
    P.set_vio_poses(0, util.poses_to_matrices(g.truth_q, g.truth_t))
    n_vio = P.add_odometry_edges_from_vio(None, 0, 10, f_max=2)
    assert n_vio == 17
    add(5, 7, ("cauchy", 1.0))
    add(7, 8, None)
    add(8, 9, ("huber", 2.5))
    kind, a = P.relpose_edge_loss()
    assert P.num_relpose_edges() == 9 + n_vio == len(kind)
    assert list(kind) == [0] * 3 + [1] * 2 + [0] * n_vio + [2] * 2 + [0] + [1]
    assert list(a) == [0.0] * 3 + [0.1] * 2 + [0.0] * n_vio + [1.0] * 2 + [0.0] + [2.5]
    kind, a = P.relpose_edge_loss(4, 2)
    assert list(kind) == [1, 0] and list(a) == [0.1, 0.0]
    with pytest.raises(capi.PgoError):
        P.relpose_edge_loss(0, P.num_relpose_edges() + 1)
    P.close()
