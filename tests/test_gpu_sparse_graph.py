"""GPU: pgo_sparse_graph of libpgo_sparse.so (csrc/pgo_sparse_graph.hpp, sparse_cholesky.Graph / solve_graph) — a pose graph that linearises itself, yaw/pitch/roll-weighted
edges included, and the exact LM solve on it without a handle.

  1. the device blocks against the 50-digit goldens, with Jacobians and cost-only;  2. the classes a handle can hold against the handle;  3. the normal blocks of every
  graph against np.longdouble products of the device's own Jacobians, within a derived rounding bound;  4. the device against the host instantiation
  (tests/native/sparse_graph_host.cpp), and two linearisations bit for bit;  5. solves: against the CPU checker, against the host instantiation's solve with
  yaw/pitch/roll loop closures below and above the dense limit, and bit for bit twice;  6. the contract.

The graphs (tests/sparse_graph_cases.py) are the smallest at which the kernels can go wrong: fewer blocks than a wave, exactly 256 and 257 blocks (the workgroup boundary of
the block kernel and of the cost tree), an incident list longer than a workgroup, empty classes.  Every test prints its figures (`SPARSEGRAPH ...`) before it asserts;
profiles/sparse_graph_check.txt records them."""
import functools

import numpy as np
import pytest

from solve_keyframe_pose_graph_amd import capi, graphgen
from solve_keyframe_pose_graph_amd import sparse_cholesky as sc
from tests import precond_cases as pc
from tests import sparse_graph_cases as gc
from tests import util

pytestmark = pytest.mark.gpu

BOUND = gc.BOUND
GRAPHS = {"nine": gc.nine, "b256": gc.b256, "b257": gc.b257, "hub300": gc.hub300, "relonly": gc.relonly, "gold60": lambda: gc.gold60()[0], "gold40": lambda: gc.gold40()[0]}


@pytest.fixture(scope="module")
def shim():
    return gc.load_shim()


@functools.lru_cache(maxsize=None)
def spec_of(name):
    return GRAPHS[name]()


def device(spec, ypr=True):
    return gc.build(spec, sc.Graph(spec.n), ypr=ypr)


def s_of(spec):
    return spec.s if len(spec.sw) else None


def jacobians(G):
    return {kind: G.jacobian_blocks(kind) for kind in range(3)}


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 1. the device blocks against the goldens
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_relative_pose_blocks_against_the_goldens():
    spec, cases = gc.gold60()
    G = device(spec)
    cost, res, _ = G.evaluate(spec.q, spec.t, None)
    J1, J2, _ = G.jacobian_blocks(0)
    cost_only, res_only, _ = G.evaluate(spec.q, spec.t, None, want_gradient=False)
    worst = 0.0
    for k, c in enumerate(cases):
        for got, want in ((res[6 * k:6 * k + 6], np.array(c["r"])), (J1[k], np.array(c["J1"])), (J2[k], np.array(c["J2"]))):
            worst = max(worst, gc.close_enough(got, want))
    print("SPARSEGRAPH device yaw/pitch/roll relative-pose blocks against 60 goldens: worst block error / max(1, |block|) %.3e" % worst)
    assert worst <= BOUND
    assert np.array_equal(res_only, res) and cost_only == cost      # the cost-only form: the same residual bits
    assert abs(cost - 0.5 * float(res @ res)) <= 1e-13 * cost
    G.close()


def test_switchable_blocks_against_the_goldens():
    spec, cases = gc.gold40()
    G = device(spec)
    cost, res, _ = G.evaluate(spec.q, spec.t, spec.s)
    J1, J2, Js = G.jacobian_blocks(1)
    cost_only, res_only, _ = G.evaluate(spec.q, spec.t, spec.s, want_gradient=False)
    worst = 0.0
    for k, c in enumerate(cases):
        for got, want in zip((res[7 * k:7 * k + 7], J1[k], J2[k], Js[k]), gc.golden_blocks(c)):
            worst = max(worst, gc.close_enough(got, want))
    print("SPARSEGRAPH device switchable yaw/pitch/roll blocks against 40 goldens: worst block error / max(1, |block|) %.3e" % worst)
    assert worst <= BOUND
    assert np.array_equal(res_only, res) and cost_only == cost
    G.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 2. the classes a handle can hold
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_sixdof_classes_against_the_handle():
    """hub300 with its yaw/pitch/roll edges taken as SixDOFError: plain, Huber and switchable (plain and Huber) edges, regularisers, a constant keyframe"""
    spec = spec_of("hub300")
    G = device(spec, ypr=False)
    Pb = gc.handle_of(spec)
    cost, res, _ = G.evaluate(spec.q, spec.t, spec.s)
    cost_h, res_h, _ = Pb.evaluate(spec.q, spec.t, spec.s)
    worst = 0.0
    for kind in range(3):
        mine, theirs = G.jacobian_blocks(kind), Pb.jacobian_blocks(kind)
        for a, b in zip(mine[:3 if kind == 1 else 2 if kind == 0 else 1], theirs):
            for x, y in zip(a, b):
                worst = max(worst, np.abs(x - y).max() / np.abs(y).max())
    rows = np.concatenate([np.repeat(np.arange(len(spec.rel)), 6), len(spec.rel) + np.repeat(np.arange(len(spec.sw)), 7), len(spec.rel) + len(spec.sw) + np.repeat(np.arange(len(spec.reg)), 6)])
    big = np.zeros(spec.blocks); np.maximum.at(big, rows, np.abs(res_h))
    worst_r = float((np.abs(res - res_h) / big[rows]).max())
    print("SPARSEGRAPH hub300 as SixDOFError against the handle: worst Jacobian block %.3e, worst residual block %.3e, cost %.3e (relative to each block's largest entry)"
          % (worst, worst_r, abs(cost - cost_h) / cost_h))
    assert worst <= 1e-12 and worst_r <= 1e-12 and abs(cost - cost_h) <= 1e-12 * cost_h
    Pb.close(); G.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 3. the normal blocks of every graph
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_normal_blocks_are_the_products_of_the_devices_own_jacobians(name):
    spec = spec_of(name)
    G = device(spec)
    cost, res, grad = G.evaluate(spec.q, spec.t, s_of(spec))
    got = G.normal_blocks()
    values, bounds = gc.products(spec, jacobians(G), res)
    ratios = [gc.bound_ratio(g, v, b) for g, v, b in zip(got, values, bounds)]
    print("SPARSEGRAPH %-7s %4d blocks (%d yaw/pitch/roll): worst |error| / ((k + 1) u sum|a||b|) of diag %.3f grad %.3f offdiag %.3f sw_c %.3f sw_hss %.3f sw_gs %.3f"
          % (name, spec.blocks, sum(e[4] is not None for e in spec.rel + spec.sw), *ratios))
    assert max(ratios) <= 1.0
    N = spec.n
    assert np.array_equal(grad[:6 * N].reshape(N, 6), got[1])
    gs = np.zeros(grad.size - 6 * N); gs[[e[3] for e in spec.sw]] = got[5]
    assert np.array_equal(grad[6 * N:], gs)
    for node in spec.constant:
        assert not got[0][node].any() and not got[1][node].any()
    assert all(np.array_equal(d, d.T) for d in got[0])
    assert np.isfinite(cost) and all(np.isfinite(a).all() for a in got)
    G.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 4. the device against the host instantiation
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def linearisation(G, spec):
    cost, res, grad = G.evaluate(spec.q, spec.t, s_of(spec))
    out = {"cost": np.array([cost]), "residuals": res, "gradient": grad}
    out.update(zip(("diag", "grad", "offdiag", "sw_c", "sw_hss", "sw_gs"), G.normal_blocks()))
    for kind in range(3):
        out.update(zip(("J1 of kind %d" % kind, "J2 of kind %d" % kind, "dr_ds of kind %d" % kind), G.jacobian_blocks(kind)))
    out["plus"] = np.concatenate([a.reshape(-1) for a in G.manifold_plus(spec.q, spec.t, 0.1 * np.cos(np.arange(6.0 * spec.n)))])
    return out


def test_the_kernels_against_the_host_instantiation(shim):
    spec = spec_of("hub300")
    G, H = device(spec), gc.build(spec, gc.HostGraph(shim, spec.n))
    a, h = linearisation(G, spec), linearisation(H, spec)
    worst = {k: float(np.abs(a[k] - h[k]).max() / max(np.abs(h[k]).max(), 1e-300)) for k in h if h[k].size}
    print("SPARSEGRAPH hub300 device against the host instantiation, relative to each array's largest magnitude: " + "  ".join("%s %.2e" % kv for kv in worst.items()))
    assert max(worst.values()) <= 1e-12
    G.evaluate(spec.q + 0.01, spec.t, s_of(spec), want_gradient=False)      # a cost-only evaluation elsewhere in between leaves the linearisation alone
    assert all(np.array_equal(x, y) for x, y in zip(G.normal_blocks(), [a[k] for k in ("diag", "grad", "offdiag", "sw_c", "sw_hss", "sw_gs")]))
    b = linearisation(G, spec)
    assert all(np.array_equal(a[k], b[k]) for k in a), "a second linearisation at the same point gives other bits"
    G.close(); H.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 5. solves
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def same_trajectory(what, sumo, sump):
    """tests/test_gpu_sparse_lm.py's check: the same decisions, costs within 1e-8"""
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


@pytest.mark.parametrize("name,perturb,seed", [("C1", 0.0, 0), ("C1F5", 1.0, 2)])
def test_the_solve_tracks_the_cpu_checker(name, perturb, seed):
    g = graphgen.config(name)
    q, t, s = util.initial_state(g, True, perturb=perturb, seed=seed)
    _, _, _, sumo = util.oracle_problem(g, True).solve(q, t, s)
    if perturb:      # rejected steps in the checker's own log, with accepted ones on both sides
        assert [sumo.iterations[k].step_is_successful for k in range(6)] == [1, 1, 1, 0, 0, 1]
    G = sc.Graph.from_pose_graph(g, True)
    tm = {}
    _, _, _, sums = sc.solve_graph(G, q, t, s, timings=tm)
    worst = same_trajectory(name, sumo, sums)
    direct_records(sums)
    print("SPARSEGRAPH trajectory %-5s %d keyframes  %d iterations (%d unsuccessful)  worst relative cost difference to the checker %.3e  final cost %.9e  %d tiles of L"
          % (name, g.n_poses, sums.num_iterations, sums.num_unsuccessful_steps, worst, sums.final_cost, tm["info"]["l_tiles"]))
    assert sums.termination_type == sumo.termination_type
    G.close()


def against_the_host_solve(shim, what, g, switchable, loss):
    spec = gc.from_pose_graph(g, switchable, loop_gains=gc.GAINS, loop_loss=loss)
    H = gc.build(spec, gc.HostGraph(shim, spec.n))
    qh, th, sh, sumh, min_h = H.solve(spec.q, spec.t, spec.s)
    assert min_h.min() >= gc.COS80, (what, min_h.min())      # the condition: |pitch error| <= 80 degrees at every point the host evaluates
    G = sc.Graph.from_pose_graph(g, switchable, loop_gains=gc.GAINS, loop_loss=loss)
    qd, td, sd, sumd = sc.solve_graph(G, spec.q, spec.t, spec.s)
    worst = same_trajectory(what, sumh, sumd)
    direct_records(sumd)
    dt = np.abs(td - th).max()
    dr = util.rot_angle(qd.reshape(-1, 4), qh.reshape(-1, 4)).max()
    print("SPARSEGRAPH %s: %d iterations (%d unsuccessful), termination %d, cost %.6e -> %.9e, worst relative cost difference to the host solve %.3e, max |dt| %.3e, max rotation %.3e, "
          "least cos(pitch error) %.4f" % (what, sumd.num_iterations, sumd.num_unsuccessful_steps, sumd.termination_type, sumd.initial_cost, sumd.final_cost, worst, dt, dr, min_h.min()))
    assert sumd.termination_type == sumh.termination_type and sumd.num_unsuccessful_steps == sumh.num_unsuccessful_steps
    assert sumd.final_cost < sumd.initial_cost
    G.close(); H.close()


@pytest.mark.parametrize("loss", [gc.HUBER, None], ids=["huber", "trivial"])
@pytest.mark.parametrize("switchable", [True, False], ids=["switchable", "plain"])
def test_yaw_pitch_roll_loop_closures_against_the_host_solve(shim, switchable, loss):
    against_the_host_solve(shim, "tl200 %s %s" % ("switchable" if switchable else "plain", "Huber(0.1)" if loss else "trivial"), pc.graph("tl200"), switchable, loss)


def test_yaw_pitch_roll_loop_closures_above_the_dense_limit(shim):
    g = graphgen.generate(1100, 110, odom_f_max=5, seed=7)
    assert g.n_poses > capi.DENSE_MAX_KEYFRAMES
    against_the_host_solve(shim, "g1100 switchable Huber(0.1)", g, True, gc.HUBER)


def test_two_solves_on_fresh_objects_give_the_same_bits():
    g = pc.graph("tl200")
    q, t, s = util.initial_state(g, True)
    outs = []
    for _ in range(2):
        G = sc.Graph.from_pose_graph(g, True, loop_gains=gc.GAINS, loop_loss=gc.HUBER)
        outs.append(sc.solve_graph(G, q, t, s))
        G.close()
    (qa, ta, sa, ma), (qb, tb, sb, mb) = outs
    assert np.array_equal(qa, qb) and np.array_equal(ta, tb) and np.array_equal(sa, sb)
    assert ma.num_logged == mb.num_logged and ma.num_logged > 1
    assert [ma.iterations[k].cost for k in range(ma.num_logged)] == [mb.iterations[k].cost for k in range(mb.num_logged)]


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 6. the contract
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def refused(f, code=gc.ERR_INVALID_ARG):
    with pytest.raises(capi.PgoError) as e:
        f()
    assert e.value.code == code, e.value
    assert ":" in str(e.value) and len(str(e.value)) > 20      # the text of pgo_sparse_last_error
    return str(e.value)


def test_the_contract_on_the_device_object():
    n = 6
    G = sc.Graph(n)
    T = np.eye(4).flatten(order="F")
    G.add_relpose_edges([0, 1], [1, 2], [T, T], [1.0, 1.0], gains=[(0, 0, 0), gc.GAINS])
    gc.contract_cases(G, n, refused)
    q, t = np.tile([0, 0, 0, 1.0], (n, 1)), np.zeros((n, 3))
    assert "finalize" in refused(lambda: G.evaluate(q, t, np.ones(2)), gc.ERR_STATE)
    refused(lambda: G.edge_lists(), gc.ERR_STATE)
    G.set_node_regularizers([0], [T], [1.0])
    G.finalize()
    refused(lambda: G.add_relpose_edges([0], [1], [T], [1.0]), gc.ERR_STATE)
    refused(lambda: G.add_switchable_edges([0], [1], [T], [7]), gc.ERR_STATE)
    refused(lambda: G.normal_blocks(), gc.ERR_STATE)
    refused(lambda: G.jacobian_blocks(0), gc.ERR_STATE)
    refused(lambda: G.evaluate(q, t, np.ones(1)))
    refused(lambda: G.evaluate(q[:5], t[:5], np.ones(2)))
    e = G.edge_lists()      # the refusals added nothing: two relative-pose edges, one switchable edge on switch 1
    assert e["rel_c1"].tolist() == [0, 1] and e["sw_c1"].tolist() == [2] and e["sw_idx"].tolist() == [1] and e["n_switch"] == 2
    assert e["in_system"].tolist() == [1, 1, 1, 1, 0, 0] and sorted(zip(e["pair_hi"].tolist(), e["pair_lo"].tolist())) == [(1, 0), (2, 1), (3, 2)]
    cost, res, grad = G.evaluate(q, t, np.ones(2))
    assert res.size == 2 * 6 + 7 + 6 and grad.size == 6 * n + 2 and np.isfinite(cost)
    refused(lambda: G.jacobian_blocks(0, 1, 2))
    refused(lambda: G.jacobian_blocks(3))
    assert [a.shape for a in G.jacobian_blocks(1)] == [(1, 6, 6), (1, 6, 6), (1, 7)]
    G.close()


def test_solve_exact_through_a_handle_gives_what_solve_graph_gives():
    g = graphgen.config("C1")
    q, t, s = util.initial_state(g, True)
    _, _, _, sumo = util.oracle_problem(g, True).solve(q, t, s)
    Pb = util.pgo_problem(g, True)
    qe, te, se, sume = sc.solve_exact(Pb, sc.Edges.from_graph(g), q, t, s)
    Pb.close()
    G = sc.Graph.from_pose_graph(g, True)
    qg, tg, sg, sumg = sc.solve_graph(G, q, t, s)
    G.close()
    worst_o, worst = same_trajectory("solve_exact against the checker", sumo, sume), same_trajectory("solve_graph against solve_exact", sume, sumg)
    direct_records(sume); direct_records(sumg)
    print("SPARSEGRAPH C1: solve_exact against the checker %.3e, solve_graph against solve_exact %.3e (worst relative cost difference), max |dt| %.3e" % (worst_o, worst, np.abs(tg - te).max()))
    assert sumg.termination_type == sume.termination_type == sumo.termination_type
    assert np.abs(tg - te).max() <= 1e-6 and util.rot_angle(qg.reshape(-1, 4), qe.reshape(-1, 4)).max() <= 1e-6
