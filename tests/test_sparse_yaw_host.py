"""CPU: the linearisation of pgo_sparse_yaw_graph (csrc/pgo_sparse_yaw_math.hpp) through its host instantiation (tests/native/sparse_yaw_host.cpp) — the same per-item
functions in the same orders as the kernels of csrc/pgo_sparse_yaw.hpp, and the whole exact solve (sc_lm_solve over ScLmHost) on them: the reference's 4-DoF (yaw +
translation) solve without a GPU.

  1. the edge (reference QinFourDOFWeightError) against 50-digit goldens (tests/golden/yaw_goldens.json), and the numpy model of tests/yaw_model.py against the same; bound
     1e-12 x max(1, largest |entry| of the block), the project's for functor blocks; NormalizeAngle as it is;
  2. the host normal blocks against np.longdouble products of the host's own Jacobians within (k + 1) u sum |a||b|, the pad entries and the symmetry exactly;
  3. the plus with wrap-around;
  4. whole solves: against a second minimiser (scipy least_squares over tests/yaw_model.py), and through +-180 degrees against the same graph rotated by 90 degrees;
  5. the contract: every PGO_ERR_INVALID_ARG and PGO_ERR_STATE of the interface, on the validation the device object runs too (SyGraph);
  6. the stand-alone program under the sanitizers; the library's symbols and sources."""
import dataclasses
import os
import subprocess

import numpy as np
import pytest
import scipy.optimize

from tests import sparse_yaw_cases as yc
from tests import yaw_model as ym

BOUND = yc.BOUND
DP = yc.dp
# _build.source_tree_hash() of the parent commit, computed once from an export of that commit: libpgo.so is built from what it was built from
PARENT_SOURCE_HASH = "16a9da9d6934f805b6c9f52e6a79aa94e806ecc6dce44a870b14794d88bd6603"


@pytest.fixture(scope="module")
def shim():
    return yc.load_shim()


def host_edge(lib, c):
    xi, xj, rec = yc.F64(c["xi"]), yc.F64(c["xj"]), yc.F64(c["rec"])
    r, J1, J2 = np.zeros(4), np.zeros((4, 4)), np.zeros((4, 4))
    lib.syh_residual(yc.P(xi, DP), yc.P(xj, DP), yc.P(rec, DP), yc.P(r, DP), yc.P(J1, DP), yc.P(J2, DP))
    return r, J1, J2


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 1. the edge against goldens
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_goldens_keep_their_conditions():
    cases = yc.golden()
    assert len(cases) == 73 and sum(c["tag"] == "random" for c in cases) == 60
    assert [c["yaw_argument"] for c in cases[:7]] == [179.9, 180.0, 180.1, -180.0, -180.1, 400.0, 800.0]
    assert [c["xi"][0] for c in cases if c["tag"].startswith("psi_i")] == [0.0, 90.0, -90.0]
    assert sum(c["xi"][1:] == c["xj"][1:] for c in cases) == 2
    assert all(abs(c["rec"][4]) <= 60 and abs(c["rec"][5]) <= 60 for c in cases) and max(abs(c["rec"][4]) for c in cases) > 50
    yaws = [c["xi"][0] for c in cases if c["tag"] == "random"]
    assert min(yaws) < -170 and max(yaws) > 170


def test_normalize_angle_is_the_references_single_fold(shim):
    for a, want in ((179.9, 179.9), (180.0, 180.0), (180.1, 180.1 - 360.0), (-180.0, -180.0), (-180.1, 360.0 - 180.1), (400.0, 40.0), (800.0, 440.0), (-800.0, -440.0), (0.0, 0.0)):
        assert shim.syh_normalize(a) == want and float(ym.normalize_angle(a)) == want, a


def test_host_edge_matches_the_goldens(shim):
    worst = 0.0
    for c in yc.golden():
        for got, want in zip(host_edge(shim, c), (c["r"], c["J1"], c["J2"])):
            e = yc.close_enough(got, want)
            worst = max(worst, e)
            assert e <= BOUND, (c["tag"], e)
    print("SPARSEYAW host edge against the goldens: worst error / max(1, |block|) %.3e" % worst)


def test_numpy_model_matches_the_goldens():
    worst = 0.0
    for c in yc.golden():
        rec = np.array(c["rec"])
        state_yaw, state_t = np.array([c["xi"][0], c["xj"][0]]), np.array([c["xi"][1:], c["xj"][1:]])
        r = ym.residuals(np.array([0]), np.array([1]), rec[None, :3], rec[3:4], rec[4:5], rec[5:6], rec[6:7], state_yaw, state_t)[0]
        worst = max(worst, yc.close_enough(r, c["r"]))
    print("SPARSEYAW numpy model against the goldens: worst %.3e" % worst)
    assert worst <= BOUND


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 2. the host normal blocks
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(yc.GRAPHS))
def test_host_normal_blocks_are_the_products_of_the_hosts_own_jacobians(shim, name):
    spec = yc.GRAPHS[name]()
    H = yc.build(spec, yc.HostGraph(shim, spec.n))
    cost, res, grad = H.evaluate(spec.yaw, spec.t)
    blocks = H.normal_blocks()
    J1, J2 = H.jacobian_blocks()
    e = H.edge_lists()
    ratios = yc.check_normal_blocks(spec, blocks, J1, J2, res, e["in_system"])
    print("SPARSEYAW host %-10s %4d edges: worst |error| / ((k + 1) u sum|a||b|) of diag %.3f grad %.3f offdiag %.3f" % (name, spec.edges, *ratios))
    assert max(ratios) <= 1.0
    assert np.array_equal(grad.reshape(-1, 6), blocks[1])
    want = ym.residuals(spec.c1, spec.c2, spec.t_meas, spec.rel_yaw, spec.pitch_i, spec.roll_i, spec.w, spec.yaw, spec.t).reshape(-1)
    assert yc.close_enough(res, want) <= BOUND and abs(cost - 0.5 * float(want @ want)) <= 1e-12 * cost
    cost_only, res_only, _ = H.evaluate(spec.yaw, spec.t, want_gradient=False)
    assert cost_only == cost and np.array_equal(res_only, res)
    referenced = np.zeros(spec.n, bool); referenced[spec.c1] = True; referenced[spec.c2] = True
    free = np.ones(spec.n, bool); free[list(spec.constant)] = False
    assert np.array_equal(e["in_system"] != 0, referenced & free) and np.array_equal(e["node_free"] != 0, free)
    H.close()


def test_edge_lists_of_duplicate_edges_and_a_graph_without_a_free_keyframe(shim):
    spec = yc.duplicates()
    H = yc.build(spec, yc.HostGraph(shim, spec.n))
    e = H.edge_lists()
    pairs = list(zip(e["pair_hi"].tolist(), e["pair_lo"].tolist()))
    assert pairs == sorted(set(pairs)) and (3, 2) in pairs and (6, 4) in pairs and all(hi > lo for hi, lo in pairs)
    assert np.array_equal(e["c1"], spec.c1) and np.array_equal(e["c2"], spec.c2)
    H.close()
    fixed = dataclasses.replace(spec, constant=tuple(range(spec.n)))
    H = yc.build(fixed, yc.HostGraph(shim, spec.n))
    cost, res, grad = H.evaluate(spec.yaw, spec.t)
    diag, g, off = H.normal_blocks()
    assert np.isfinite(cost) and cost > 0 and not grad.any() and not diag.any() and len(H.edge_lists()["pair_hi"]) == 0
    y, t, sm, _ = H.solve(spec.yaw, spec.t)      # an empty system: nothing moves
    assert np.array_equal(y, spec.yaw) and np.array_equal(t, spec.t) and sm.final_cost == cost
    H.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 3. the plus
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_plus_wraps_the_yaw_and_keeps_the_layout(shim):
    H = yc.HostGraph(shim, 8)
    yaw = np.array([170.0, -170.0, 0.0, 180.0, -180.0, 10.0, 179.0, -90.0])
    t = np.arange(24.0).reshape(8, 3)
    d = np.zeros((8, 6))
    d[:, 0] = [20.0, -20.0, 5.0, 0.0, 0.0, 400.0, 1.0, -90.0]
    d[:, 3:] = 0.25
    d[:, 1:3] = 7.0      # whatever the pad entries of a delta hold, they move nothing
    y1, t1 = H.manifold_plus(yaw, t, d)
    assert y1.tolist() == [-170.0, 170.0, 5.0, 180.0, -180.0, 50.0, 180.0, -180.0]
    assert np.array_equal(t1, t + 0.25)
    y2, none = H.manifold_plus(yaw, None, d)      # the controller's call: t = NULL
    assert none is None and np.array_equal(y2, y1)
    H.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 4. whole solves
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
SOLVE = dict(max_num_iterations=200, function_tolerance=1e-14, parameter_tolerance=1e-12)


def chain12(seed, **kw):
    """12 keyframes, a chain with skips of 1 - 2, three loop closures, keyframe 0 constant, noisy measurements and a noisy start"""
    return yc.synthetic(12, yc.chain_pairs(12) + [(0, 8), (10, 2), (11, 4)], seed, constant=(0,), weights=False, **kw)


def test_host_solve_agrees_with_scipy_least_squares(shim):
    """the condition, asserted by the model at every point scipy evaluates and here at every point the host evaluates: |psi_j - psi_i - rel_yaw| < 90 on every edge —
    no fold anywhere near, the problem is smooth"""
    spec = chain12(21, turn=4.0, yaw0=-20.0)
    assert spec.edges == 21 + 3 and spec.constant == (0,)
    H = yc.build(spec, yc.HostGraph(shim, spec.n))
    yh, th, sm, far = H.solve(spec.yaw, spec.t, **SOLVE)
    assert sm.termination_type == 0
    assert far.max() < 90.0, far.max()
    N = spec.n

    def state(x):
        z = x.reshape(N - 1, 4)
        return np.concatenate([spec.yaw[:1], spec.yaw[1:] + z[:, 0]]), np.concatenate([spec.t[:1], spec.t[1:] + z[:, 1:]])

    def fun(x):
        return ym.residuals(spec.c1, spec.c2, spec.t_meas, spec.rel_yaw, spec.pitch_i, spec.roll_i, spec.w, *state(x), smooth_below=90.0).reshape(-1)
    c0, r0, _ = H.evaluate(spec.yaw, spec.t, want_gradient=False)
    assert np.abs(r0 - fun(np.zeros(4 * (N - 1)))).max() <= 1e-12 * max(1.0, np.abs(r0).max())
    res = scipy.optimize.least_squares(fun, np.zeros(4 * (N - 1)), method="trf", x_scale="jac", xtol=1e-14, ftol=1e-14, gtol=1e-12, max_nfev=400)
    y, t = state(res.x)
    dy, dt = np.abs(y - yh).max(), np.linalg.norm(t - th, axis=1).max()
    print("SPARSEYAW host 4-DoF solve against scipy: %d iterations, cost %.6e -> %.12e (scipy %.12e), max |dyaw| %.3e degrees, max |dt| %.3e, largest yaw argument %.2f degrees"
          % (sm.num_iterations, sm.initial_cost, sm.final_cost, res.cost, dy, dt, far.max()))
    assert sm.final_cost < 0.5 * sm.initial_cost
    assert abs(res.cost - sm.final_cost) <= 1e-8 * sm.final_cost
    assert dy <= 1e-4 and dt <= 1e-4
    H.close()


def test_host_solve_through_the_wrap_matches_the_graph_rotated_by_a_quarter_turn(shim):
    """a trajectory that turns through +-180 degrees, with edges straddling the wrap, must reach the cost of the same graph rotated by 90 degrees about z: the start's yaws
    + 90 (folded), its translations rotated; the edge records — relative yaw, t_meas, pitch and roll — left as they are, since they are body-frame"""
    spec = chain12(22, turn=15.0, yaw0=60.0)

    def straddling(s):
        return np.abs(s.yaw[s.c2] - s.yaw[s.c1] - s.rel_yaw) > 180.0
    Rz = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    turned = dataclasses.replace(spec, yaw=ym.normalize_angle(spec.yaw + 90.0), t=spec.t @ Rz.T)
    assert straddling(spec).sum() >= 3 and straddling(turned).sum() >= 3 and (straddling(spec) != straddling(turned)).sum() >= 6      # other edges straddle after the turn
    out = []
    for s in (spec, turned):
        H = yc.build(s, yc.HostGraph(shim, s.n))
        y, t, sm, far = H.solve(s.yaw, s.t, **SOLVE)
        assert sm.termination_type == 0 and far.max() > 180.0 and np.abs(y).max() <= 180.0
        out.append((y, t, sm))
        H.close()
    (ya, ta, sa), (yb, tb, sb) = out
    print("SPARSEYAW host solve through the wrap: cost %.6e -> %.12e in %d iterations; rotated by 90 degrees %.12e in %d iterations; max |dyaw| %.3e, max |dt| %.3e"
          % (sa.initial_cost, sa.final_cost, sa.num_iterations, sb.final_cost, sb.num_iterations, np.abs(ym.normalize_angle(yb - ya - 90.0)).max(), np.abs(tb - ta @ Rz.T).max()))
    assert sa.final_cost < 0.5 * sa.initial_cost
    assert abs(sa.initial_cost - sb.initial_cost) <= 1e-8 * sa.initial_cost
    assert abs(sa.final_cost - sb.final_cost) <= 1e-8 * sa.final_cost


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 5. the contract
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def refused(f, code=yc.ERR_INVALID_ARG):
    with pytest.raises(yc.HostError) as e:
        f()
    assert e.value.code == code, e.value
    return str(e.value)


def test_the_contract_on_the_host_validation(shim):
    n = 6
    G = yc.HostGraph(shim, n)
    G.add_edges([0, 1], [1, 2], [[1.0, 0, 0], [1.0, 0, 0]], [5.0, 5.0], [1.0, 2.0], [3.0, 4.0])
    yc.contract_cases(G, n, refused)
    yaw, t = np.zeros(n), np.zeros((n, 3))
    assert "finalize" in refused(lambda: G.evaluate(yaw, t), yc.ERR_STATE)                            # evaluated before finalize
    refused(lambda: G.edge_lists(), yc.ERR_STATE)
    G.finalize()
    refused(lambda: G.add_edges([0], [1], [[1.0, 0, 0]], [5.0], [1.0], [2.0]), yc.ERR_STATE)           # edges added after finalize
    refused(lambda: G.set_nodes_constant([1]), yc.ERR_STATE)
    refused(lambda: G.normal_blocks(), yc.ERR_STATE)                                                  # no linearisation yet
    refused(lambda: G.jacobian_blocks(), yc.ERR_STATE)
    refused(lambda: G.evaluate(yaw[:5], t[:5]))                                                       # n_nodes is not the graph's
    for slot in (1, 2, 3):                                                                            # a state whose quat slots 1 - 3 are not 0
        q = yc.pack(yaw); q[4, slot] = 1e-300
        assert "slots" in refused(lambda: G.evaluate_packed(q, t))
    refused(lambda: G.normal_blocks(), yc.ERR_STATE)
    cost, res, grad = G.evaluate(yaw, t)                                                              # the refusals left the object usable and added nothing: two edges
    assert G.edge_lists()["c1"].tolist() == [0, 1] and res.size == 8 and grad.size == 6 * n and np.isfinite(cost)
    assert not grad[6 * 3:].any() and G.edge_lists()["in_system"].tolist() == [1, 1, 1, 0, 0, 0]
    refused(lambda: G.jacobian_blocks(1, 2))
    refused(lambda: G.jacobian_blocks(-1, 1))
    assert [a.shape for a in G.jacobian_blocks(1)] == [(1, 4, 4), (1, 4, 4)]
    G.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 6. the same code in a sanitized stand-alone program; the library's new symbols and sources
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_stand_alone_program_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "sparse_yaw_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DSYH_MAIN"] + yc.INCLUDES + ["-o", exe, yc.SRC])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr


def test_the_entry_points_are_declared_exported_and_beside_the_library():
    import ctypes
    from solve_keyframe_pose_graph_amd import _build
    txt = open(os.path.join(yc.ROOT, "include", "pgo_sparse.h")).read()
    names = [n for n in _build.SPARSE_EXPORTS if n.startswith("pgo_sparse_yaw_")]
    assert len(names) == 12 and _build.SPARSE_EXPORTS[-12:] == names
    lib = ctypes.CDLL(_build.build_libpgo_sparse())
    for name in names:
        assert hasattr(lib, name) and (" %s(" % name) in txt, name
    assert _build.SPARSE_HEADERS[-2:] == ["pgo_sparse_yaw.hpp", "pgo_sparse_yaw_math.hpp"] and not set(_build.SPARSE_HEADERS[-2:]) & set(_build.HIP_HEADERS)
    assert "pgo_sparse" not in " ".join(_build.HIP_SOURCES)
    assert _build.source_tree_hash() == PARENT_SOURCE_HASH      # libpgo.so is built from what it was built from
