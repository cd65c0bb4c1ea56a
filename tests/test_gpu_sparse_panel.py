"""GPU: the columns of the inverse in number of libpgo_sparse.so (csrc/pgo_sparse.hip: sc_pcol_rhs_kernel, sc_pfwd_kernel, sc_pbwd_kernel, sc_pgather_kernel;
pgo_sparse_chol_{inverse_columns, columns_info, set_workspace_limit}) and sparse_cholesky.cross_covariance / loop_candidate_gate on top of them.

  1. the kernels on the matrices of tests/test_sparse_selinv_host.py, entered as 6 x 6 block systems, natural order and permuted, against the refined inverse AND
  against the host instantiation on the very same plan;  2. equal bits: alone, in a batch, in chunks, twice, and the factor untouched;  3. the blocks of the
  40-keyframe system, the pair (5, 30) that the selected inverse refuses among them;  4. a graph above PGO_DENSE_MAX_KEYFRAMES: pairs outside the factor's pattern
  against tests/sparse_cov_ref.py and against sparse_cholesky.covariance;  5. cross_covariance on block-CSR and matrix-free handles against Problem.covariance;
  6. the gate;  7. the contract.

Error measure and bound: tests/test_sparse_panel_host.py's — the scaled entrywise e, MARGIN x e_np; two device paths against each other 2 x that.  Device against host
is held to the bound, not to equal bits: the MFMA adds the four products of a step in another order.  Every test prints its figures (`SPARSE panel ...`) before it
asserts."""
import functools

import numpy as np
import pytest

from solve_keyframe_pose_graph_amd import capi, graphgen
from solve_keyframe_pose_graph_amd import sparse_cholesky as sc
from tests import param_cov_ref as pref
from tests import precond_cases as pc
from tests import sparse_cov_ref as sref
from tests import util
from tests.pose_cov_cases import LOOPS
from tests.test_sparse_panel_host import (GATHER_N, GATHER_REQUEST, MARGIN, NAMES, PERMUTED, HostColumns, as_block_system, check_block_gather, gather_case, load_shim, permuted_matrix, reference,
                                          same_bits, scaled, whole_inverse_blocks)

pytestmark = pytest.mark.gpu

BLOCK_CSR, MATRIX_FREE = capi.LINEAR_PCG_BLOCK_JACOBI, capi.LINEAR_PCG_MATRIX_FREE
CHI2_6_999 = 22.46      # the 0.999 quantile of chi-square with 6 degrees of freedom


@pytest.fixture(scope="module")
def shim():
    return load_shim()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 1. the kernels against the reference and the host instantiation
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def check_kernels(tag, shim, A, S_ref, S_np, ordering):
    n = len(A)
    N, hi, lo, diag, blocks = as_block_system(A)
    ins = np.ones(N, np.uint8)
    F = sc.SparseCholesky(N, ins, hi, lo, ordering)
    F.factor(diag, blocks)
    X = whole_inverse_blocks(F, N)
    ms, info = F.last_ms(), F.columns_info()
    again = whole_inverse_blocks(F, N)
    F.close()
    H = HostColumns(shim, N, ins, hi, lo, ordering)
    assert H.h and H.factor(diag, blocks)
    X_host = whole_inverse_blocks(H, N)
    host_info = H.columns_info()
    H.close()
    d = np.sqrt(np.diag(S_ref).astype(np.float64))
    e, e_np, e_host = scaled(X[:n, :n], S_ref), scaled(S_np, S_ref), float((np.abs(X[:n, :n] - X_host[:n, :n]) / np.outer(d, d)).max())
    print("SPARSE panel kernels %-24s n %3d  launches %2d  products %3d  workspace %7d B  e %.3e  e_np %.3e  e / e_np %.2f  against the host %.3e  equal bits: %s  %.3f ms"
          % (tag, n, info["launches"], info["tile_products"], info["bytes"], e, e_np, e / e_np, e_host, same_bits(X, X_host), ms))
    assert info == host_info and info["chunks"] == 1      # the plan's counts
    assert same_bits(X, again)                            # two calls give the same bits
    pad = np.arange(n, 6 * N)                             # the identity rows that fill the last block: exactly 1 on the diagonal, 0 elsewhere
    assert np.all(X[pad][:, pad] == np.eye(len(pad))) and np.all(X[pad, :n] == 0.0) and np.all(X[:n, pad] == 0.0)
    assert e <= MARGIN * e_np
    assert e_host <= MARGIN * e_np


@pytest.mark.parametrize("name", NAMES)
def test_kernels_in_natural_order(shim, name):
    A, S_ref, S_np = reference(name)
    check_kernels(name, shim, A, S_ref, S_np, sc.ORDER_NATURAL)


@pytest.mark.parametrize("name", PERMUTED)
def test_kernels_under_a_permutation_of_the_nodes(shim, name):
    """the nodes of the matrix permuted before it goes in (the library's own orders are natural and reverse Cuthill-McKee), and reverse Cuthill-McKee on top"""
    A, S_ref, S_np = reference(name, True)
    _, pos = permuted_matrix(name)
    inv = np.argsort(pos)      # row q of the permuted matrix is row inv[q] of A
    take = lambda M: np.asarray(M)[np.ix_(inv, inv)]
    check_kernels(name + " permuted", shim, take(A), take(S_ref), take(S_np), sc.ORDER_NATURAL)
    check_kernels(name + " permuted, rcm", shim, take(A), take(S_ref), take(S_np), sc.ORDER_RCM)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 2. bits
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ordering", [sc.ORDER_NATURAL, sc.ORDER_RCM])
def test_a_column_gets_the_same_bits_alone_in_a_batch_and_in_chunks_and_the_factor_survives(ordering):
    ins, hi, lo, diag, blocks, A, _ = gather_case()
    N = GATHER_N
    F = sc.SparseCholesky(N, ins, hi, lo, ordering)
    F.factor(diag, blocks)
    nt = F.info()[0]["nt"]
    b = np.random.default_rng(4).standard_normal(6 * N)
    x = F.solve(b)
    F.selected_inverse()
    marginals, _ = F.selected_blocks(np.arange(N), np.arange(N))
    rows = np.arange(N)
    alone = F.inverse_columns([10], rows, np.zeros(N, np.int32)).reshape(6 * N, 6)
    one = F.columns_info()
    batch = whole_inverse_blocks(F, N)
    whole = F.columns_info()
    twice = whole_inverse_blocks(F, N)
    F.set_workspace_limit(64 * 64 * nt * 8)      # one panel: ten keyframes per chunk
    chunked = whole_inverse_blocks(F, N)
    parts = F.columns_info()
    after = F.solve(b)
    marginals_after, _ = F.selected_blocks(np.arange(N), np.arange(N))
    F.close()
    print("SPARSE panel bits ordering %d: alone %s  all 40 columns %s  in chunks %s  alone = batch: %s  batch = chunked: %s  solve before = after: %s"
          % (ordering, one, whole, parts, same_bits(alone, batch[:, 60:66]), same_bits(batch, chunked), same_bits(x, after)))
    assert one["chunks"] == 1 and whole["chunks"] == 1 and parts["chunks"] >= 3 and parts["bytes"] <= 64 * 64 * nt * 8 < whole["bytes"]
    assert same_bits(alone, batch[:, 60:66]) and same_bits(batch, twice) and same_bits(batch, chunked)
    assert same_bits(x, after) and same_bits(marginals, marginals_after)      # the factor and the selected inverse are only read


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 3. the gather
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ordering", [sc.ORDER_NATURAL, sc.ORDER_RCM])
def test_blocks_of_any_pair_on_the_40_keyframe_system(shim, ordering):
    ins, hi, lo, diag, blocks, A, R = gather_case()
    F = sc.SparseCholesky(GATHER_N, ins, hi, lo, ordering)
    F.factor(diag, blocks)
    F.selected_inverse()
    _, flag = F.selected_blocks([5, 10], [30, 10])
    out = check_block_gather("kernels, ordering %d" % ordering, F, ins, R)
    F.close()
    H = HostColumns(shim, GATHER_N, ins, hi, lo, ordering)
    assert H.h and H.factor(diag, blocks)
    want = check_block_gather("host, ordering %d" % ordering, H, ins, R)
    H.close()
    d = np.sqrt(np.diag(np.linalg.inv(A)))
    apart = max(float((np.abs(out[k] - want[k]) / np.outer(d[6 * a:6 * a + 6], d[6 * b:6 * b + 6])).max()) for k, (a, b) in enumerate(GATHER_REQUEST))
    print("SPARSE panel gather ordering %d: the selected inverse has (5, 30): %s  kernels against the host %.3e  bound %.3e" % (ordering, bool(flag[0]), apart, R.bound))
    assert flag[1] and (ordering != sc.ORDER_NATURAL or not flag[0])      # natural order, a band: the selected inverse refuses (5, 30) — and check_block_gather held it to the bound
    assert apart <= R.bound


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 4. above the dense limit
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
PAIRS_1100 = [(1099, j) for j in range(0, 1000, 100)] + [(i + 550, i) for i in range(0, 501, 50)]
PAIRS_WIDE = [(i, i + 550) for i in range(0, 500, 5)]      # 100 distinct keyframes on either side: cross_covariance serves them by the panel sweeps, PAIRS_1100 (12 columns) by the solve


@functools.lru_cache(maxsize=None)
def g1100():
    """the 1 100-keyframe graph of tests/test_gpu_sparse_cholesky.py, its state and its handle's normal blocks"""
    g = graphgen.generate(1100, 110, odom_f_max=5, seed=7)
    assert g.n_poses > capi.DENSE_MAX_KEYFRAMES and len(g.reg_node) > 0
    q, t, s = pc.state(g)
    return g, q, t, s, sc.Edges.from_graph(g, True)


def test_cross_covariance_above_the_dense_limit():
    g, q, t, s, ed = g1100()
    N = g.n_poses
    assert len(PAIRS_1100) == 21
    P = util.pgo_problem(g, True, linear_solver=BLOCK_CSR)
    got, other, outside, tms, direct = {}, {}, {}, {}, {}
    for ordering in (sc.ORDER_NATURAL, sc.ORDER_RCM):
        tms[ordering] = {}
        got[ordering] = sc.cross_covariance(P, ed, q, t, s, PAIRS_1100, ordering=ordering, timings=tms[ordering])
        other[ordering] = sc.covariance(P, ed, q, t, s, PAIRS_1100, ordering=ordering)
    tm_wide = {}
    wide = sc.cross_covariance(P, ed, q, t, s, PAIRS_WIDE, ordering=sc.ORDER_RCM, timings=tm_wide)
    nb = P.normal_blocks()
    P.close()
    diag, _, off, c, hss, _ = nb
    free = np.ones(N, np.uint8)
    hi, lo, sd, sb = sc.reduce_normal_blocks(N, free, diag, off, c, hss, ed.rel_c1, ed.rel_c2, ed.sw_c1, ed.sw_c2)
    for ordering in (sc.ORDER_NATURAL, sc.ORDER_RCM):
        F = sc.SparseCholesky(N, free, hi, lo, ordering)
        F.factor(sd, sb)
        F.selected_inverse()
        _, flag = F.selected_blocks([a for a, _ in PAIRS_1100], [b for _, b in PAIRS_1100])
        direct[ordering] = sc.cross_blocks(F, PAIRS_1100)      # the kernels themselves, whatever cross_covariance's routing
        F.close()
        outside[ordering] = int((~flag).sum())
    R = sref.Reference(N, free.astype(bool), free.astype(bool), nb, ed.rel_c1, ed.rel_c2, ed.sw_c1, ed.sw_c2, PAIRS_1100)
    R_wide = sref.Reference(N, free.astype(bool), free.astype(bool), nb, ed.rel_c1, ed.rel_c2, ed.sw_c1, ed.sw_c2, PAIRS_WIDE[::10])
    e_wide = R_wide.error(wide[::10])
    print("SPARSE panel g1100 rcm, %d pairs with %d column keyframes: served by %s in %.2f ms (%s)  every tenth against the reference: e %.3e  e_np %.3e  bound 8 e_np %.3e"
          % (len(PAIRS_WIDE), len(PAIRS_WIDE), tm_wide["route"], tm_wide["columns_ms"], tm_wide["columns_info"], e_wide, R_wide.e_np, R_wide.bound))
    for ordering in (sc.ORDER_NATURAL, sc.ORDER_RCM):
        tm = tms[ordering]
        e, e_other = R.error(got[ordering]), R.error(other[ordering])
        between = max(float((np.abs(x - y) / np.sqrt(np.outer(R.var_at[a], R.var_at[b]))).max()) for (a, b), x, y in zip(PAIRS_1100, got[ordering], other[ordering]))
        print("SPARSE panel g1100 ordering %d  tiles of L %4d  outside the pattern %2d of 21  factor %.2f ms  blocks by %s %.2f ms  e %.3e  (the kernels %.3e, covariance() %.3e, between the two %.3e)  e_np %.3e  bound 8 e_np %.3e"
              % (ordering, tm["info"]["l_tiles"], outside[ordering], tm["factor_ms"], tm["route"], tm["columns_ms"], e, R.error(direct[ordering]), e_other, between, R.e_np, R.bound))
    for ordering in (sc.ORDER_NATURAL, sc.ORDER_RCM):
        assert outside[ordering] >= 10      # (the host plan: 11 in natural order, all 21 under reverse Cuthill-McKee)
        assert got[ordering].shape == (21, 6, 6) and np.isfinite(got[ordering]).all()
        assert R.error(got[ordering]) <= R.bound, ordering
        assert R.error(direct[ordering]) <= R.bound, ordering
        assert tms[ordering]["route"] == "solve"      # 12 column keyframes: below sparse_cholesky.SOLVE_BELOW_COLUMNS
        between = max(float((np.abs(x - y) / np.sqrt(np.outer(R.var_at[a], R.var_at[b]))).max()) for (a, b), x, y in zip(PAIRS_1100, got[ordering], other[ordering]))
        assert between <= 2.0 * R.bound, ordering
    assert len(PAIRS_WIDE) == sc.SOLVE_BELOW_COLUMNS and tm_wide["route"] == "columns" and wide.shape == (len(PAIRS_WIDE), 6, 6)
    assert e_wide <= R_wide.bound


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 5. cross_covariance where pgo_covariance also runs
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
N24 = 24
PAIRS_24 = [(0, 22), (22, 0), (1, 17), (9, 9), (2, 20), (20, 2), (10, 11), (11, 10), (4, 9), (9, 23), (4, 4), (0, 0), (23, 23), (10, 10), (5, 19)]


@pytest.mark.parametrize("solver, constant", [(BLOCK_CSR, ()), (MATRIX_FREE, ()), (BLOCK_CSR, (4, 23))])
def test_cross_covariance_on_24_keyframes(solver, constant):
    g = pref.with_loops(N24, LOOPS)
    q, t, s = pc.state(g)
    P = util.pgo_problem(g, True, linear_solver=solver)
    if len(constant):
        P.set_nodes_constant(np.asarray(constant, dtype=np.int32))
    ed = sc.Edges.from_graph(g, True, constant)
    got = sc.cross_covariance(P, ed, q, t, s, PAIRS_24)
    again = sc.cross_covariance(P, ed, q, t, s, PAIRS_24)
    dense = P.covariance(q, t, s, PAIRS_24)
    free = np.ones(N24, bool); free[np.asarray(constant, dtype=np.int64)] = False
    H, rows_of = pref.handle_full_matrix(P, g, free)
    with pytest.raises(ValueError):
        sc.cross_covariance(P, ed, q, t, s, [(0, N24)])      # out of range
    P.close()
    live = [k for k, (a, b) in enumerate(PAIRS_24) if free[a] and free[b]]
    R = pref.FullReference(H, [PAIRS_24[k] for k in live], rows_of)
    e, e_dense = R.error([got[k] for k in live]), R.error([dense[k] for k in live])
    between = max(float((np.abs(got[k] - dense[k]) / np.sqrt(np.outer(R.var[R.at[PAIRS_24[k][0]]], R.var[R.at[PAIRS_24[k][1]]]))).max()) for k in live)
    print("SPARSE panel cross 24 keyframes, solver %d, constant %s: %d pairs  e %.3e  (pgo_covariance %.3e, between the two %.3e)  e_np %.3e  bound 8 e_np %.3e" % (solver, constant, len(PAIRS_24), e, e_dense, between, R.e_np, R.bound))
    assert got.shape == (len(PAIRS_24), 6, 6) and same_bits(got, again)
    pref.check_exact_structure(PAIRS_24, got)
    assert all(np.all(got[k] == 0.0) for k in range(len(PAIRS_24)) if k not in live) and (len(live) < len(PAIRS_24)) == (len(constant) > 0)
    assert e <= R.bound
    assert between <= 2.0 * R.bound


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 6. the gate
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
NEAR = [(106, 100), (406, 400), (806, 800), (1006, 1000)]      # six keyframes apart: the odometry edges reach five
FAR = [(1099, 0), (1099, 500), (600, 50)]
GATE_WEIGHT = 10.0


def test_the_gate_passes_the_estimates_own_relative_pose_and_rejects_it_displaced():
    """Candidates that are NOT edges of the 1 100-keyframe graph, weight 10 (a measurement good to 0.1 in the graph's units, whose own edges carry weights 0.59 .. 1).
    Their measurement is first the estimate's own relative pose — r = 0, d^2 = 0 — and then the same displaced by 5 along x.  What 5 is worth depends on how well the
    posterior ties the two keyframes: d^2 ~ 25 / (sigma^2 + 1 / weight^2) for a relative variance sigma^2 along the displacement.
      * NEAR, (i + 6, i): five two-edge odometry paths i -> i + f -> i + 6 join them, of variances 1 / w^2 summed over the two edges — 4.1, 3.84, 3.76, 3.84, 4.1 with
        the generator's weights 0.9^f — so sigma^2 <= 1 / (2 / 4.1 + 2 / 3.84 + 1 / 3.76) = 0.79 and d^2 >= 25 / 0.80 = 31 > 22.46: the gate must reject.  ASSERTED.
      * FAR pairs hundreds of keyframes apart hang on a chain of such edges and a few loop closures of weight 1: sigma^2 is of the order of 1e2 (the variances of this
        graph reach 7e2, tests/test_gpu_sparse_cholesky.py) and 5 is inside the noise; the gate cannot reject and nothing is asserted of their d^2: printed."""
    g, q, t, s, ed = g1100()
    edges = set(zip(g.odom_c1.tolist(), g.odom_c2.tolist())) | set(zip(g.loop_c1.tolist(), g.loop_c2.tolist()))
    cand = NEAR + FAR
    assert not any((a, b) in edges or (b, a) in edges for a, b in cand) and g.odom_w.min() > 0.59 and g.odom_w.max() <= 0.9
    c1, c2 = np.array([a for a, _ in cand], np.int32), np.array([b for _, b in cand], np.int32)
    near = np.arange(len(NEAR))
    M = util.poses_to_matrices(q, t).reshape(-1, 4, 4).transpose(0, 2, 1)
    own = np.stack([np.linalg.inv(M[a]) @ M[b] for a, b in cand])      # the estimate's own relative poses
    moved = own.copy(); moved[:, 0, 3] += 5.0                          # ... displaced by 5
    as16 = lambda T: np.ascontiguousarray(T.transpose(0, 2, 1)).reshape(-1, 16)
    w = np.full(len(cand), GATE_WEIGHT)
    P = util.pgo_problem(g, True, linear_solver=BLOCK_CSR)
    tm = {}
    G0 = sc.loop_candidate_gate(P, ed, q, t, s, c1, c2, as16(own), w, timings=tm)
    G5 = sc.loop_candidate_gate(P, ed, q, t, s, c1, c2, as16(moved), w)
    cross = sc.cross_covariance(P, ed, q, t, s, np.stack([c1, c2], axis=1))
    P.close()
    eig = np.array([np.linalg.eigvalsh(S).min() for S in np.concatenate([G0.innovation_cov, G5.innovation_cov])])
    print("SPARSE panel gate g1100: weight %.3g  factor %.2f ms  selected inverse %.2f ms  columns %.2f ms (%s)" % (w[0], tm["factor_ms"], tm["selected_ms"], tm["columns_ms"], tm["columns_info"]))
    print("SPARSE panel gate g1100: candidates %s" % cand)
    print("SPARSE panel gate g1100: own relative pose  |r| %s  d^2 %s" % (np.array2string(np.abs(G0.residual).max(axis=1), precision=2), np.array2string(G0.mahalanobis2, precision=3)))
    print("SPARSE panel gate g1100: displaced by 5     |r| %s  d^2 %s  (chi^2_6 0.999: %.2f; asserted of the first %d)  smallest eigenvalue of S %.3f"
          % (np.array2string(np.abs(G5.residual).max(axis=1), precision=3), np.array2string(G5.mahalanobis2, precision=2), CHI2_6_999, len(NEAR), eig.min()))
    n = len(cand)
    assert G0.residual.shape == (n, 6) and G0.cross.shape == (n, 6, 6) and G0.innovation_cov.shape == (n, 6, 6) and G0.mahalanobis2.shape == (n,)
    assert np.all(G0.mahalanobis2 >= 0.0) and np.all(G0.mahalanobis2 <= 1e-20)
    assert np.all(G5.mahalanobis2[near] > CHI2_6_999)
    assert all(np.array_equal(S, S.T) for S in G0.innovation_cov) and all(np.array_equal(S, S.T) for S in G5.innovation_cov) and np.all(eig > 0.0)
    assert same_bits(G0.cross, cross) and same_bits(G0.cross, G5.cross)      # the gate's cross-covariances are cross_covariance's
    for G in (G0, G5):
        again = np.array([r @ np.linalg.solve(S, r) for r, S in zip(G.residual, G.innovation_cov)])
        assert np.all(np.abs(G.mahalanobis2 - again) <= 1e-12 * np.maximum(np.abs(again), 1e-300))


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 7. the contract
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_call_order_counts_and_refusals(shim):
    ins, hi, lo, diag, blocks, A, _ = gather_case()
    N = GATHER_N
    F = sc.SparseCholesky(N, ins, hi, lo, sc.ORDER_RCM)
    nt = F.info()[0]["nt"]
    with pytest.raises(capi.PgoError) as err:
        F.inverse_columns([10], [5], [0])
    assert err.value.code == sc.ERR_STATE      # no factor yet
    assert F.columns_info() == dict(zip(sc.COLUMNS_INFO, [0, 0, 0, 0]))
    F.factor(diag, blocks)
    H = HostColumns(shim, N, ins, hi, lo, 1)
    assert H.h and H.factor(diag, blocks)
    requests = [([10], [5], [0]), ([30, 2, 17], [0, 38, 20, 20], [0, 0, 1, 2]), ([3, 39], [10, 3], [0, 1]), (np.arange(N), np.arange(N)[::-1].copy(), np.arange(N))]
    for cn, rn, ci in requests:
        got, want = F.inverse_columns(cn, rn, ci), H.inverse_columns(cn, rn, ci)
        print("SPARSE panel contract: %2d columns %2d blocks  %s  last_ms %.3f" % (len(cn), len(rn), F.columns_info(), F.last_ms()))
        assert F.columns_info() == H.columns_info() and np.allclose(got, want, rtol=0, atol=1e-12)
        assert F.last_ms() > 0.0
    assert F.columns_info()["chunks"] == 1
    got = F.inverse_columns([3, 39], [10, 3], [0, 1])      # keyframes outside the system alone: nothing to solve, zero blocks
    assert np.all(got == 0.0) and F.columns_info() == dict(zip(sc.COLUMNS_INFO, [0, 0, 0, 0]))
    for cn, rn, ci in (([N], [5], [0]), ([-1], [5], [0]), ([10], [N], [0]), ([10, 10], [5], [0]), ([10], [5], [1]), ([10], [5], [-1])):
        cn_, rn_, ci_ = sc._i(cn), sc._i(rn), sc._i(ci)
        keep = np.full((len(rn_), 36), 7.0)
        rc = F.lib.pgo_sparse_chol_inverse_columns(F.h, len(cn_), sc._p(cn_, sc._ip), len(rn_), sc._p(rn_, sc._ip), sc._p(ci_, sc._ip), sc._p(keep, sc._dp))
        assert rc == sc.ERR_INVALID_ARG and np.all(keep == 7.0), (cn, rn, ci)
    with pytest.raises(capi.PgoError) as err:
        F.set_workspace_limit(64 * 64 * nt * 8 - 1)      # below one panel
    assert err.value.code == sc.ERR_INVALID_ARG
    F.set_workspace_limit(64 * 64 * nt * 8)
    H.set_workspace_limit(64 * 64 * nt * 8)
    cn, rn, ci = requests[-1]
    F.inverse_columns(cn, rn, ci); H.inverse_columns(cn, rn, ci)
    assert F.columns_info() == H.columns_info() and F.columns_info()["chunks"] >= 3
    H.close()
    bad = diag.copy(); bad[5] = -np.eye(6)      # not positive definite: a failed factor leaves no factor
    with pytest.raises(capi.PgoError) as err:
        F.factor(bad, blocks)
    assert err.value.code == sc.ERR_NUMERIC
    with pytest.raises(capi.PgoError) as err:
        F.inverse_columns([10], [5], [0])
    assert err.value.code == sc.ERR_STATE
    F.close()
