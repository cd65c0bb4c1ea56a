"""GPU: the LM normal operator — matrix-free (mf_spmv_kernel) and assembled (build_rows_kernel + apply_operator_kernel) — as a dense matrix at the edges of the tile
packing, K2's per-keyframe sums on the same tiles, the grid-stride trips of the matvec beyond MF_MAX_GRID tiles, and the fused PCG forms on these tiles, against the
sparse fp64 reference of tests/normal_operator_ref.py (checked on the CPU, with its teeth, in tests/test_normal_operator_ref.py).

A slot or lane error in the packing gives a wrong 6 x 6 block in a few rows; PCG then converges to a slightly wrong step and LM still descends, so cost-level tests
have little chance of seeing it.  Here the operator is extracted column by column (pgo_apply_normal_operator_batch with X = I, one call) and compared entry by entry.

The tile tables come from the device (pgo_get_matrix_free_tiles): a matrix-free test asserts that it RAN matrix-free and that the tile it aims at exists — as properties
(a tile with 256 lanes, a tile without lanes, ...), not as exact boundaries, so a later repacking keeps these tests and must only keep the edge cases reachable.

Contract for keyframes outside the system (constant, or referenced by no residual block), read off build_rows_kernel and the two matvecs and asserted here exactly
and identically in both forms:
  * the six ROWS of such a keyframe are identity rows: exactly 1.0 on the diagonal, exactly 0.0 everywhere else (the damping plane of the matrix-free form holds 1.0
    there and its row phase skips the edge sums; the assembled form writes the identity block and zero coupling blocks);
  * its COLUMNS are not masked: the rows of its free neighbours keep their coupling block with it, equal to the reference's block as if it were free — every PCG
    vector is zero in those rows, so the solver never multiplies the block by anything else; an unreferenced keyframe has no neighbours, its columns are unit vectors;
  * the diagonal blocks of its free neighbours keep the J^T J and switch terms of the edges to it.

Tolerances: 1e-10 of |A_ref|max is the project's operator tolerance (tests/test_gpu_parity.py); per 6 x 6 block 1e-10 max(|A_ii|max, |A_jj|max); K2 at
test_normal_matrix_matches_oracle's 1e-11; the PCG iterates at the bound tests/test_gpu_precond_operator.py::check_iterate derives (8 x the model's own
fp32-against-fp64 block-Jacobi difference + 1e-9 |x_k|).  Every test prints `NORMALOP ...` lines before it asserts; profiles/normal_operator_check.txt records them."""
import ctypes as C

import numpy as np
import pytest

from solve_keyframe_pose_graph_amd import capi
from tests import normal_operator_cases as nc
from tests import normal_operator_ref as nr
from tests import solve_digest, util

pytestmark = pytest.mark.gpu

PGO_ERR_INVALID_ARG, PGO_ERR_STATE = -1, -5
FORM_NAMES = {0: "assembled", 1: "matrix-free"}
NO_MULTIGRID = dict(mg_min_keyframes=10 ** 9, mg_min_keyframes_switchable=10 ** 9, mg_switch_iterations=0, coarse_aggregates=0)


def open_solve(G, **opt):
    P = nc.pgo_problem(G, **opt)
    q, t, s = nc.state(G)
    P.solve_begin(q, t, s)
    return P


def check_tiles(P, G, linear_solver, condition="case"):
    """the device's tile tables: none for the assembled operator (asked for, or the fall-back); else the invariants of any packing and the case's target condition"""
    T = P.matrix_free_tiles()
    if linear_solver == 0 or not G.matrix_free:
        assert T["n_tiles"] == 0, T["n_tiles"]
        return T
    assert T["n_tiles"] > 0
    nr.tile_invariants(T, G.n_poses)
    cond = G.condition if condition == "case" else condition
    assert nr.tile_condition(T, cond), (cond, T["lanes"], np.diff(T["node0"]))
    sw_lanes = T["lanes"] - T["first_switch_lane"]
    assert np.all(T["first_switch_lane"] >= T["pair_lanes"]) and np.all(sw_lanes >= 0) and sw_lanes.sum() == 2 * G.n_sw      # a switchable edge: one lane per side
    assert T["sides"].sum() == 2 * (len(G.rel_c1) + G.n_sw)
    return T


def tiles_text(T):
    return "tiles %d (max lanes %d, min lanes %d, max sides %d)" % (T["n_tiles"], T["lanes"].max(), T["lanes"].min(), T["sides"].max()) if T["n_tiles"] else "tiles 0"


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# dense extraction
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", nc.RADII)
@pytest.mark.parametrize("name", nc.SMALL)
def test_dense_operator_in_both_forms(name, radius):
    G = nc.graph(name)
    N = G.n_poses
    A_ref, _, free = nr.device_rows(nc.reference(name, radius), G.constant)
    A_ref = A_ref.toarray()
    norm = np.abs(A_ref).max()
    frows = np.flatnonzero(np.repeat(free, 6))
    orows = np.flatnonzero(~np.repeat(free, 6))
    got, figures = {}, {}
    for ls in (0, 1):
        P = open_solve(G, linear_solver=ls, initial_trust_region_radius=radius)
        T = check_tiles(P, G, ls)
        A = P.apply_normal_operator_batch(np.eye(6 * N), radius).T.copy()      # column v of A is the image of unit vector v
        P.solve_end(); P.close()
        c = nr.compare(A, A_ref)
        Af = A[np.ix_(frows, frows)]
        asym = float(np.abs(Af - Af.T).max() / norm)
        print("NORMALOP dense %-20s %-11s radius %.0e  %s  |A_dev - A_ref| %.3e  per block %.3e  asymmetry %.3e  non-zeros outside the pattern %d" %
              (name, FORM_NAMES[ls] if T["n_tiles"] or ls == 0 else "fall-back", radius, tiles_text(T), c["err"], c["err_block"], asym, c["nonzero_outside"]))
        got[ls], figures[ls] = A, (c, asym)
    agree = float(np.abs(got[0] - got[1]).max() / norm)
    print("NORMALOP forms %-20s radius %.0e  |A_assembled - A_matrix-free| %.3e" % (name, radius, agree))
    want_rows = np.zeros((len(orows), 6 * N)); want_rows[np.arange(len(orows)), orows] = 1.0
    for ls in (0, 1):
        c, asym = figures[ls]
        assert np.isfinite(got[ls]).all()
        assert c["err"] <= 1e-10 and c["err_block"] <= 1e-10, (ls, c)
        assert c["nonzero_outside"] == 0                                   # blocks of keyframe pairs that share no edge: exactly 0.0
        assert asym <= 1e-13
        assert np.array_equal(got[ls][orows], want_rows)                   # keyframes outside the system: identity rows, exactly
    assert agree <= 1e-12


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# K2 on the same tiles
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("linear_solver", [0, 1])
@pytest.mark.parametrize("name", nc.SMALL)
def test_k2_sums_on_the_same_tiles(name, linear_solver):
    """normal_blocks() — k2_tiles_kernel walks the matvec's tile tables under the matrix-free solver, k2_node_kernel the incident lists otherwise — against the reference's
    undamped sum J^T J blocks, J^T r, and the off-diagonal sums per keyframe pair (parallel and reversed edges added up)"""
    G = nc.graph(name)
    ref = nc.reference(name, nc.RADII[0])
    q, t, s = nc.state(G)
    P = nc.pgo_problem(G, linear_solver=linear_solver)
    P.evaluate(q, t, s)
    T = check_tiles(P, G, linear_solver)
    diag, grad, off, _, _, _ = P.normal_blocks()
    P.close()
    hmax = max(1.0, np.abs(ref.diag).max(), max(np.abs(b).max() for b in ref.pair_off.values()))
    gmax = max(1.0, np.abs(ref.grad).max())
    e_diag = float(np.abs(diag - ref.diag).max() / hmax)
    e_grad = float(np.abs(grad - ref.grad).max() / gmax)
    acc = {}
    c1 = np.concatenate([G.rel_c1, G.sw_c1]); c2 = np.concatenate([G.rel_c2, G.sw_c2])
    for e in range(len(c1)):
        key = (int(c1[e]), int(c2[e]))
        acc[key] = acc.get(key, 0.0) + off[e]
    assert set(acc) == set(ref.pair_off)
    e_off = max(float(np.abs(acc[k] - ref.pair_off[k]).max() / hmax) for k in acc)
    n_par = sum(1 for (a, b) in acc if (b, a) in acc) // 2
    print("NORMALOP k2    %-20s %-11s %s  |Hd - ref| %.3e  |g - ref| %.3e  |sum J1^T J2 - ref| %.3e  (%d pairs, %d in both orientations)" %
          (name, FORM_NAMES[linear_solver] if T["n_tiles"] or linear_solver == 0 else "fall-back", tiles_text(T), e_diag, e_grad, e_off, len(acc), n_par))
    assert e_diag <= 1e-11 and e_grad <= 1e-11 and e_off <= 1e-11


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# more than MF_MAX_GRID tiles: the matvec's grid-stride loop
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def big_vectors(T, N):
    """8 vectors: six random ones and the indicators of the keyframes the workgroups serve on their first and on their second trip (every tile when the operator is assembled:
    the split by the Python rule's tables)"""
    rng = np.random.default_rng(0)
    X = rng.normal(size=(8, 6 * N))
    split = 6 * int(T["node0"][nr.MF_MAX_GRID])
    X[6] = 0.0; X[6, :split] = 1.0
    X[7] = 0.0; X[7, split:] = 1.0
    return X


def test_more_tiles_than_workgroups():
    """small_graph(44000, 4400, f=1): more than 1 024 tiles and not a multiple of it, so some workgroups of mf_spmv_kernel make two trips and the others one; the second trip
    re-reads the tile bounds and its input from memory instead of the registers preloaded for the first"""
    G = nc.big_graph()
    N, radius = G.n_poses, nc.RADII[0]
    A, _, free = nr.device_rows(nc.reference("big44000", radius), G.constant)
    assert free.all()
    got = {}
    rule = nr.tile_rule(N, G.rel_c1, G.rel_c2, G.sw_c1, G.sw_c2)
    scale = None
    for ls in (1, 0):
        P = open_solve(G, linear_solver=ls, initial_trust_region_radius=radius, **NO_MULTIGRID)
        T = check_tiles(P, G, ls, condition=None)
        if ls == 1:
            assert T["n_tiles"] > nr.MF_MAX_GRID and T["n_tiles"] % nr.MF_MAX_GRID != 0, T["n_tiles"]
            X = big_vectors(T, N)
        Y = P.apply_normal_operator_batch(X, radius)
        P.solve_end(); P.close()
        Y_ref = (A @ X.T).T
        err = float(np.abs(Y - Y_ref).max() / np.abs(Y_ref).max())
        scale = nr.row_block_scale(A, X) if scale is None else scale
        delta = np.abs(Y - Y_ref).reshape(len(X), N, 6).max(axis=2)
        live = scale > 0.0      # (the indicator vectors: a keyframe whose row blocks meet only zeros of x has the exact image 0)
        rel_rows = float((delta[live] / scale[live]).max()) if np.all(delta[~live] == 0.0) else np.inf
        second = slice(6 * int((T if ls == 1 else rule)["node0"][nr.MF_MAX_GRID]), None)
        err_second = float(np.abs(Y[:, second] - Y_ref[:, second]).max() / np.abs(Y_ref).max())
        print("NORMALOP big   %-20s %-11s radius %.0e  %s  8 vectors  |y_dev - y_ref| %.3e  per keyframe row block %.3e  rows of the second trip %.3e" %
              (G.name, FORM_NAMES[ls], radius, tiles_text(T), err, rel_rows, err_second))
        got[ls] = (Y, err, rel_rows)
    agree = float(np.abs(got[0][0] - got[1][0]).max() / np.abs(got[1][0]).max())
    print("NORMALOP forms %-20s radius %.0e  |y_assembled - y_matrix-free| %.3e" % (G.name, radius, agree))
    for ls in (0, 1):
        assert np.isfinite(got[ls][0]).all()
        assert got[ls][1] <= 1e-10 and got[ls][2] <= 1e-10, (ls, got[ls][1:])
    assert agree <= 1e-12


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# the fused forms on these tiles: x_k of a k-step block-Jacobi PCG
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
FORMS = {
    # label: (options, single-reduction form expected, linear_solver)
    "classic matrix-free": (dict(cg_single_reduction=0), 0, 1),      # mf_spmv_kernel<FUSED>: p = z + beta p_prev formed inside the matvec
    "single-reduction":    (dict(), 1, 1),
    "assembled":           (dict(linear_solver=0), 0, 0),
}
KS = (1, 2, 3)


def iterate(G, k, radius, handle=None, **opt):
    """tests/precond_child.py::linear_iterate's recipe on a graph of these cases: pauses off, no multigrid, no two-level method, cg_max_iterations = k"""
    base = dict(cg_early_tolerance=0.0, cg_mid_tolerance=0.0, initial_trust_region_radius=radius, cg_max_iterations=k, **NO_MULTIGRID)
    base.update(opt)
    if handle is None:
        handle = nc.pgo_problem(G, **base)
    else:
        handle.set_options(**base)
    q, t, s = nc.state(G)
    handle.solve_begin(q, t, s)
    handle.lm_step()
    x = handle.linear_solution()
    _, _, _, sm = handle.solve_end()
    return x, sm.iterations[1], handle


def check_iterates(name, G, label, radius):
    opt, sr, ls = FORMS[label]
    A, b, free = nr.device_rows(nc.reference(name, radius), G.constant)
    D = nr.diagonal_blocks(A)
    x64 = nr.pcg(A, b, nr.block_jacobi_factors(D), max(KS))
    x32 = nr.pcg(A, b, nr.block_jacobi_factors(D, fp32=True), max(KS))
    outside = ~np.repeat(free, 6)
    P, rows = None, []
    for k in KS:
        x, it, P = iterate(G, k, radius, handle=P, **opt)
        T = check_tiles(P, G, ls, condition="case" if name != "big44000" else None)
        if name == "big44000" and ls == 1:
            assert T["n_tiles"] > nr.MF_MAX_GRID and T["n_tiles"] % nr.MF_MAX_GRID != 0
        tol = 8 * np.abs(x32[k - 1] - x64[k - 1]).max() + 1e-9 * np.abs(x64[k - 1]).max()      # test_gpu_precond_operator.py::check_iterate's bound
        dev = float(np.abs(x - x64[k - 1]).max())
        print("NORMALOP iterate %-18s %-20s radius %.0e  %s  k %d  |x_k - x_k(ref)| %.3e  tolerance %.3e  |x_k| %.3e" %
              (name, label, radius, tiles_text(T), k, dev, tol, np.abs(x64[k - 1]).max()))
        rows.append((k, x, it, dev, tol))
    P.close()
    for k, x, it, dev, tol in rows:
        assert it.cg_iterations == k and it.preconditioner == capi.PRECOND_BLOCK_JACOBI and it.single_reduction == sr, (it.cg_iterations, it.preconditioner, it.single_reduction)
        assert np.all(x[outside] == 0.0)
        assert dev <= tol


@pytest.mark.parametrize("radius", nc.RADII)
@pytest.mark.parametrize("label", sorted(FORMS))
@pytest.mark.parametrize("name", ["hub256", "lanes-sw", "gap"])
def test_iterates_of_the_block_jacobi_pcg_forms(name, label, radius):
    check_iterates(name, nc.graph(name), label, radius)


@pytest.mark.parametrize("label", sorted(FORMS))
def test_iterates_beyond_the_matvec_grid(label):
    """the only route to the non-first-trip loads of the FUSED matvec (z[vi] and p_prev[vi] in place of the preloaded registers)"""
    check_iterates("big44000", nc.big_graph(), label, nc.RADII[0])


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# contract of the two diagnostics
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_diagnostics_error_paths_and_the_single_vector_hook():
    G = nc.graph("boundary85")
    q, t, s = nc.state(G)
    n6 = 6 * G.n_poses
    P = nc.pgo_problem(G)
    n = C.c_int64(-1)
    dp = C.POINTER(C.c_double)
    X, Y = np.zeros(n6), np.zeros(n6)
    batch = lambda radius, n_vec, x, y: P.lib.pgo_apply_normal_operator_batch(P.h, C.c_double(radius), C.c_int64(n_vec), x.ctypes.data_as(dp) if x is not None else None, y.ctypes.data_as(dp) if y is not None else None)
    # before a graph is built / a solve is open
    assert P.lib.pgo_get_matrix_free_tiles(P.h, None, None, None, None, None, C.c_int64(0), C.byref(n)) == PGO_ERR_STATE and n.value == 0
    assert batch(0.0, 1, X, Y) == PGO_ERR_STATE and b"open solve" in P.lib.pgo_last_error(P.h)
    P.solve_begin(q, t, s)
    for radius, n_vec, x, y in ((0.0, 0, X, Y), (float("nan"), 1, X, Y), (float("inf"), 1, X, Y), (0.0, 1, None, Y), (0.0, 1, X, None)):
        assert batch(radius, n_vec, x, y) == PGO_ERR_STATE and b"invalid argument" in P.lib.pgo_last_error(P.h)
    T = P.matrix_free_tiles()
    assert T["n_tiles"] == 3
    short = np.zeros(2, np.int32)
    assert P.lib.pgo_get_matrix_free_tiles(P.h, None, short.ctypes.data_as(C.POINTER(C.c_int32)), None, None, None, C.c_int64(2), C.byref(n)) == PGO_ERR_INVALID_ARG and n.value == 3
    # radius <= 0 is the current radius, which the call leaves alone; one vector of the batch is what pgo_apply_normal_operator returns
    rng = np.random.default_rng(0)
    x = rng.normal(size=n6)
    y_cur = P.apply_normal_operator_batch(x, 0.0)
    assert np.array_equal(y_cur, P.apply_normal_operator_batch(x, 1e4)) and not np.array_equal(y_cur, P.apply_normal_operator_batch(x, 1e-2))
    assert np.array_equal(P.apply_normal_operator_batch(x, -1.0), y_cur)
    assert np.array_equal(P.apply_normal_operator(x), y_cur)
    P.solve_end(); P.close()
    P = nc.pgo_problem(G)
    P.comm_init_custom(0, 1, lambda buf, count, op, stream: 0)
    assert P.lib.pgo_get_matrix_free_tiles(P.h, None, None, None, None, None, C.c_int64(0), C.byref(n)) == PGO_ERR_STATE and b"communicator" in P.lib.pgo_last_error(P.h)
    assert batch(0.0, 1, X, Y) == PGO_ERR_STATE and b"communicator" in P.lib.pgo_last_error(P.h)
    P.comm_destroy(); P.close()


def test_a_handle_the_diagnostics_were_used_on_solves_like_a_fresh_one():
    """the two diagnostics between solve_begin and solve_end, then a solve on the same handle: every output array and the whole iteration log equal a fresh handle's, bit for bit"""
    fresh = solve_digest.digest("C1F5")
    g, switchable = solve_digest.graph("C1F5")
    q, t, s = util.initial_state(g, switchable)
    P = util.pgo_problem(g, switchable)
    P.solve_begin(q, t, s)
    assert P.matrix_free_tiles()["n_tiles"] > 0
    rng = np.random.default_rng(1)
    for radius in (0.0, 1e-2):
        assert np.isfinite(P.apply_normal_operator_batch(rng.normal(size=(3, 6 * g.n_poses)), radius)).all()
    P.solve_end()
    used = solve_digest.digest("C1F5", handle=P)
    P.close()
    assert used == fresh
