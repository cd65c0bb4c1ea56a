"""GPU: pgo_sparse_yaw_graph of libpgo_sparse.so (csrc/pgo_sparse_yaw.hpp, sparse_cholesky.YawGraph / solve_yaw_graph) — the reference's 4-DoF (yaw + translation) pose
graph that linearises itself in the six-row slots of the exact LM step, and the exact solve on it.

  1. the device edges against the 50-digit goldens, with Jacobians and cost-only;  2. the device against the host instantiation (tests/native/sparse_yaw_host.cpp), every
  array, and two linearisations bit for bit;  3. the normal blocks of every graph against np.longdouble products of the device's own Jacobians within a derived rounding
  bound, pad entries and symmetry exactly;  4. the plus against the host's, bit for bit;  5. solves against the host instantiation's solve below and above the dense limit,
  and bit for bit twice;  6. the contract;  7. the factor and the selected inverse on the undamped blocks of a solve's final linearisation.

The graphs (tests/sparse_yaw_cases.py) are the smallest at which the kernels can go wrong: fewer edges than a wave, exactly 256 and 257 edges (the workgroup boundary of the
block kernel and of the cost tree), an incident list longer than a workgroup, an unreferenced and two constant keyframes, duplicate edges.  Every test prints its figures
(`SPARSEYAW ...`) before it asserts; profiles/sparse_yaw_check.txt records them."""
import functools

import numpy as np
import pytest

from solve_keyframe_pose_graph_amd import capi, graphgen
from solve_keyframe_pose_graph_amd import sparse_cholesky as sc
from tests import precond_cases as pc
from tests import sparse_yaw_cases as yc

pytestmark = pytest.mark.gpu

BOUND = yc.BOUND


@pytest.fixture(scope="module")
def shim():
    return yc.load_shim()


@functools.lru_cache(maxsize=None)
def spec_of(name):
    return yc.GRAPHS[name]()


def device(spec):
    return yc.build(spec, sc.YawGraph(spec.n))


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 1. the device edges against the goldens
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_device_edges_against_the_goldens():
    spec, cases = yc.gold()
    G = device(spec)
    cost, res, _ = G.evaluate(spec.yaw, spec.t)
    J1, J2 = G.jacobian_blocks()
    cost_only, res_only, _ = G.evaluate(spec.yaw, spec.t, want_gradient=False)
    worst = 0.0
    for k, c in enumerate(cases):
        for got, want in ((res[4 * k:4 * k + 4], c["r"]), (J1[k], c["J1"]), (J2[k], c["J2"])):
            worst = max(worst, yc.close_enough(got, want))
    print("SPARSEYAW device edges against %d goldens: worst block error / max(1, |block|) %.3e" % (len(cases), worst))
    assert worst <= BOUND
    assert np.array_equal(res_only, res) and cost_only == cost      # the cost-only form: the same residual bits
    assert abs(cost - 0.5 * float(res @ res)) <= 1e-13 * cost
    G.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 2. the device against the host instantiation
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def linearisation(G, spec):
    cost, res, grad = G.evaluate(spec.yaw, spec.t)
    out = {"cost": np.array([cost]), "residuals": res, "gradient": grad}
    out.update(zip(("diag", "grad", "offdiag"), G.normal_blocks()))
    out.update(zip(("J1", "J2"), G.jacobian_blocks()))
    return out


@pytest.mark.parametrize("name", sorted(yc.GRAPHS))
def test_the_kernels_against_the_host_instantiation(shim, name):
    spec = spec_of(name)
    G, H = device(spec), yc.build(spec, yc.HostGraph(shim, spec.n))
    a, h = linearisation(G, spec), linearisation(H, spec)
    worst = {k: yc.close_enough(a[k], h[k]) for k in h}
    print("SPARSEYAW %-10s %4d edges, device against the host instantiation, |difference| / max(1, largest |entry|): " % (name, spec.edges) + "  ".join("%s %.2e" % kv for kv in worst.items()))
    assert max(worst.values()) <= BOUND
    e, eh = G.edge_lists(), H.edge_lists()
    assert all(np.array_equal(e[k], eh[k]) for k in eh)
    cost_only, res_only, _ = G.evaluate(spec.yaw + 1.0, spec.t, want_gradient=False)      # a cost-only evaluation elsewhere in between leaves the linearisation alone
    assert all(np.array_equal(x, a[k]) for x, k in zip(G.normal_blocks(), ("diag", "grad", "offdiag")))
    cost_only, res_only, _ = G.evaluate(spec.yaw, spec.t, want_gradient=False)
    assert cost_only == a["cost"][0] and np.array_equal(res_only, a["residuals"])          # the cost-only form: the same residual bits
    b = linearisation(G, spec)
    assert all(np.array_equal(a[k], b[k]) for k in a), "a second linearisation at the same point gives other bits"
    G.close(); H.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 3. the normal blocks of every graph
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(yc.GRAPHS))
def test_normal_blocks_are_the_products_of_the_devices_own_jacobians(name):
    spec = spec_of(name)
    G = device(spec)
    cost, res, grad = G.evaluate(spec.yaw, spec.t)
    blocks = G.normal_blocks()
    J1, J2 = G.jacobian_blocks()
    ratios = yc.check_normal_blocks(spec, blocks, J1, J2, res, G.edge_lists()["in_system"])
    print("SPARSEYAW %-10s %4d edges: worst |error| / ((k + 1) u sum|a||b|) of diag %.3f grad %.3f offdiag %.3f" % (name, spec.edges, *ratios))
    assert max(ratios) <= 1.0
    assert np.array_equal(grad.reshape(-1, 6), blocks[1])
    assert np.isfinite(cost) and all(np.isfinite(a).all() for a in blocks)
    G.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 4. the plus
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_plus_kernel_gives_the_hosts_bits(shim):
    n = 601      # more than two workgroups, not a multiple of one
    rng = np.random.default_rng(9)
    yaw = rng.uniform(-180.0, 180.0, n)
    yaw[:4] = [180.0, -180.0, 179.5, -179.5]
    t = rng.standard_normal((n, 3))
    d = rng.standard_normal((n, 6)) * [200.0, 1.0, 1.0, 0.5, 0.5, 0.5]      # folds in both directions; the pad entries of a delta move nothing
    d[:4, 0] = [0.0, 0.0, 0.5, -0.5]
    G, H = sc.YawGraph(n), yc.HostGraph(shim, n)
    (yd, td), (yh, th) = G.manifold_plus(yaw, t, d), H.manifold_plus(yaw, t, d)
    assert np.array_equal(yd, yh) and np.array_equal(td, th)
    assert yd[:4].tolist() == [180.0, -180.0, 180.0, -180.0] and np.sum(np.abs(yaw + d[:, 0]) > 180.0) > 100
    y_only, none = G.manifold_plus(yaw, None, d)      # the controller's call: t = NULL
    assert none is None and np.array_equal(y_only, yh)
    G.close(); H.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 5. solves
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def direct_records(sm):
    for k in range(1, sm.num_logged):
        it = sm.iterations[k]
        assert it.cg_iterations == 0 and it.cg_iterations_multigrid == 0 and it.cg_residual == 0.0 and it.preconditioner == capi.PRECOND_DIRECT, k
    assert sm.cg_iterations == 0 and sm.pcg_retries == 0


def against_the_host_solve(shim, what, spec, rejected):
    H = yc.build(spec, yc.HostGraph(shim, spec.n))
    yh, th, sumh, far = H.solve(spec.yaw, spec.t)
    G = device(spec)
    tm = {}
    yd, td, sumd = sc.solve_yaw_graph(G, spec.yaw, spec.t, timings=tm)
    worst = yc.same_trajectory(what, sumh, sumd)
    direct_records(sumd)
    dy, dt = np.abs(yc.ym.normalize_angle(yd - yh)).max(), np.abs(td - th).max()
    print("SPARSEYAW %s: %d iterations (%d unsuccessful), termination %d, cost %.6e -> %.9e, worst relative cost difference to the host solve %.3e, max |dyaw| %.3e degrees, max |dt| %.3e, "
          "largest yaw argument %.1f degrees, %d tiles of L" % (what, sumd.num_iterations, sumd.num_unsuccessful_steps, sumd.termination_type, sumd.initial_cost, sumd.final_cost, worst, dy, dt,
                                                               far.max(), tm["info"]["l_tiles"]))
    assert sumd.termination_type == sumh.termination_type and sumd.num_unsuccessful_steps == sumh.num_unsuccessful_steps and sumd.num_successful_steps == sumh.num_successful_steps
    assert sumd.final_cost < sumd.initial_cost and np.abs(yd).max() <= 180.0
    assert (sumh.num_unsuccessful_steps >= 1) == rejected
    G.close(); H.close()


def test_the_solve_against_the_host_solve_with_rejected_steps(shim):
    """200 keyframes, the odometry start moved by 150 degrees and 5 m (standard deviation): the host's own log has a rejected step"""
    spec = yc.perturbed_start(yc.from_pose_graph(pc.graph("tl200")), 1, 150.0, 5.0)
    against_the_host_solve(shim, "tl200 from a far start", spec, rejected=True)


def test_the_solve_against_the_host_solve_above_the_dense_limit(shim):
    g = graphgen.generate(1100, 110, odom_f_max=5, seed=7)
    assert g.n_poses > capi.DENSE_MAX_KEYFRAMES      # the tile-sparse path is the only one
    against_the_host_solve(shim, "g1100 from the odometry", yc.from_pose_graph(g), rejected=False)


def test_two_solves_on_fresh_objects_give_the_same_bits():
    g = pc.graph("tl200")
    outs = []
    for _ in range(2):
        G, yaw, t, pitch, roll = sc.YawGraph.from_pose_graph(g)
        outs.append(sc.solve_yaw_graph(G, yaw, t))
        G.close()
    (ya, ta, ma), (yb, tb, mb) = outs
    assert np.array_equal(ya, yb) and np.array_equal(ta, tb)
    assert ma.num_logged == mb.num_logged and ma.num_logged > 1 and ma.final_cost < ma.initial_cost
    assert [ma.iterations[k].cost for k in range(ma.num_logged)] == [mb.iterations[k].cost for k in range(mb.num_logged)]
    spec = yc.from_pose_graph(g)      # from_pose_graph built what the shared description says
    assert np.array_equal(yaw, spec.yaw) and np.array_equal(t, spec.t)
    T = sc.yaw_state_to_poses(yaw, t, pitch, roll)
    assert np.abs(T[:, :3, :3] - sc._quat_to_rot(g.init_q)).max() <= 1e-12 and np.array_equal(T[:, :3, 3], g.init_t)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 6. the contract
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def refused(f, code=yc.ERR_INVALID_ARG):
    with pytest.raises(capi.PgoError) as e:
        f()
    assert e.value.code == code, e.value
    assert ":" in str(e.value) and len(str(e.value)) > 20      # the text of pgo_sparse_last_error
    return str(e.value)


def test_the_contract_on_the_device_object():
    n = 6
    G = sc.YawGraph(n)
    G.add_edges([0, 1], [1, 2], [[1.0, 0, 0], [1.0, 0, 0]], [5.0, 5.0], [1.0, 2.0], [3.0, 4.0])
    yc.contract_cases(G, n, refused)
    yaw, t = np.zeros(n), np.zeros((n, 3))
    assert "finalize" in refused(lambda: G.evaluate(yaw, t), yc.ERR_STATE)
    refused(lambda: G.edge_lists(), yc.ERR_STATE)
    G.finalize()
    refused(lambda: G.add_edges([0], [1], [[1.0, 0, 0]], [5.0], [1.0], [2.0]), yc.ERR_STATE)
    refused(lambda: G.set_nodes_constant([1]), yc.ERR_STATE)
    refused(lambda: G.normal_blocks(), yc.ERR_STATE)
    refused(lambda: G.jacobian_blocks(), yc.ERR_STATE)
    refused(lambda: G.evaluate(yaw[:5], t[:5]))
    q = yc.pack(yaw); q[4, 2] = 1e-300      # a state whose quat slots 1 - 3 are not 0
    cost = sc.C.c_double(0)
    tt = t.reshape(-1)
    assert G.lib.pgo_sparse_yaw_graph_evaluate(G.h, sc._p(q, sc._dp), sc._p(tt, sc._dp), n, sc.C.byref(cost), None, None) == yc.ERR_INVALID_ARG
    assert b"slots" in G.lib.pgo_sparse_last_error(None)
    refused(lambda: G.normal_blocks(), yc.ERR_STATE)      # nothing was launched: there is still no linearisation
    e = G.edge_lists()      # the refusals added nothing: two edges
    assert e["c1"].tolist() == [0, 1] and e["c2"].tolist() == [1, 2] and e["in_system"].tolist() == [1, 1, 1, 0, 0, 0]
    assert sorted(zip(e["pair_hi"].tolist(), e["pair_lo"].tolist())) == [(1, 0), (2, 1)]
    cost, res, grad = G.evaluate(yaw, t)
    assert res.size == 8 and grad.size == 6 * n and np.isfinite(cost) and not grad[18:].any()
    refused(lambda: G.jacobian_blocks(1, 2))
    refused(lambda: G.jacobian_blocks(-1, 1))
    assert [a.shape for a in G.jacobian_blocks(1)] == [(1, 4, 4), (1, 4, 4)]
    G.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 7. the factor and the covariance calls on the undamped blocks
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_undamped_blocks_of_a_solve_factor_and_their_inverse_keeps_the_pad_identity():
    spec = spec_of("e257")
    G = device(spec)
    yaw, t, sm = sc.solve_yaw_graph(G, spec.yaw, spec.t, max_num_iterations=50)
    assert sm.termination_type == 0 and sm.final_cost < 0.5 * sm.initial_cost
    G.evaluate(yaw, t)
    diag, grad, off = G.normal_blocks()
    e = G.edge_lists()
    none = np.zeros(0, np.int32)
    hi, lo, s_diag, s_blocks = sc.reduce_normal_blocks(spec.n, e["node_free"], diag, off, np.zeros((0, 12)), np.zeros(0), e["c1"], e["c2"], none, none)
    assert np.array_equal(hi, e["pair_hi"]) and np.array_equal(lo, e["pair_lo"])
    F = sc.SparseCholesky(spec.n, e["in_system"], hi, lo)
    F.factor(s_diag, s_blocks)      # positive definite without damping: the unit pad entries
    F.selected_inverse()
    nodes = [1, 64, 128]
    blocks, in_pattern = F.selected_blocks(nodes, nodes)
    assert in_pattern.all()
    want = np.zeros((6, 6)); want[1, 1] = want[2, 2] = 1.0
    pad = np.zeros((6, 6), bool); pad[yc.PADS, :] = True; pad[:, yc.PADS] = True
    worst = max(yc.close_enough(b[pad], want[pad]) for b in blocks)
    print("SPARSEYAW e257 after a solve: the factor of the undamped blocks succeeds; pad rows and columns of three marginal covariances against the identity's %.3e" % worst)
    assert worst <= BOUND and all(np.isfinite(b).all() and np.all(np.diag(b)[yc.SLOTS] > 0) for b in blocks)
    F.close(); G.close()
