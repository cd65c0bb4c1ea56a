"""CPU: the sparse edge-by-edge reference of the normal operator (tests/normal_operator_ref.py) against the dense route, the tile conditions of the cases of
tests/normal_operator_cases.py by the Python restatement of pack_mf_tiles' closing rule, and the teeth of the comparison tests/test_gpu_normal_operator.py makes: every
deliberately wrong variant of the reference moves it by at least 1e-6, four decades above the GPU tolerance 1e-10."""
import numpy as np
import pytest

from tests import normal_operator_cases as nc
from tests import normal_operator_ref as nr


def dense_route(G, radius):
    """(A, b) as tests/test_gpu_parity.py::test_normal_operator_is_schur_complement builds A: the checker's dense H, the LM diagonal, a dense Schur complement"""
    O = nc.oracle_problem(G)
    q, t, s = nc.state(G)
    H = O.dense_normal_matrix(q, t, s)
    _, _, grad = O.evaluate(q, t, s)
    n6 = 6 * G.n_poses
    d = np.diag(H)
    scale = 1.0 / (1.0 + np.sqrt(d))
    lam = np.clip(scale ** 2 * d, 1e-6, 1e32) / radius / scale ** 2
    Hd = H + np.diag(lam)
    if Hd.shape[0] == n6:
        return Hd, -grad[:n6], H
    X = np.linalg.solve(Hd[n6:, n6:], np.column_stack([Hd[n6:, :n6], grad[n6:]]))
    return Hd[:n6, :n6] - Hd[:n6, n6:] @ X[:, :n6], -(grad[:n6] - Hd[:n6, n6:] @ X[:, n6]), H


@pytest.mark.parametrize("radius", nc.RADII)
@pytest.mark.parametrize("name", nc.SMALL)
def test_reference_equals_the_dense_route(name, radius):
    G = nc.graph(name)
    ref = nc.reference(name, radius)
    A, b, H = dense_route(G, radius)
    Ar = ref.A.toarray()
    assert np.abs(Ar - A).max() <= 1e-13 * np.abs(A).max()
    assert np.abs(ref.b - b).max() <= 1e-13 * max(np.abs(b).max(), np.abs(A).max())
    assert np.abs(Ar - Ar.T).max() <= 1e-14 * np.abs(A).max()
    # what K2 is compared with: the undamped blocks before the elimination
    N, hmax = G.n_poses, np.abs(H).max()
    for n in range(N):
        assert np.abs(ref.diag[n] - H[6 * n:6 * n + 6, 6 * n:6 * n + 6]).max() <= 1e-13 * hmax
    for (a, c), blk in ref.pair_off.items():
        both = blk + (ref.pair_off[(c, a)].T if (c, a) in ref.pair_off else 0.0)
        assert np.abs(both - H[6 * a:6 * a + 6, 6 * c:6 * c + 6]).max() <= 1e-13 * hmax


def test_device_rows_of_keyframes_outside_the_system():
    G = nc.graph("boundary85-constant")
    ref = nc.reference("boundary85-constant", nc.RADII[0])
    A, b, free = nr.device_rows(ref, G.constant)
    A = A.toarray()
    full = ref.A.toarray()
    assert not free[41] and not free[42] and free.sum() == 83
    for n in (41, 42):
        rows = slice(6 * n, 6 * n + 6)
        want = np.zeros((6, 6 * G.n_poses)); want[:, rows] = np.eye(6)
        assert np.array_equal(A[rows], want) and np.all(b[rows] == 0.0)
    rows = slice(6 * 40, 6 * 40 + 6)
    assert np.array_equal(A[rows], full[rows]) and np.abs(A[rows, 6 * 41:6 * 42]).max() > 0.0      # the free neighbour keeps its coupling with the constant keyframe
    Gg = nc.graph("gap")
    _, _, free = nr.device_rows(nc.reference("gap", nc.RADII[0]), Gg.constant)
    assert not free[100:190].any() and free[:100].all() and free[190:].all()


@pytest.mark.parametrize("name", nc.SMALL)
def test_every_case_meets_its_tile_condition_by_the_closing_rule(name):
    G = nc.graph(name)
    T = nr.tile_rule(G.n_poses, G.rel_c1, G.rel_c2, G.sw_c1, G.sw_c2)
    assert nr.matrix_free_eligible(G.n_poses, G.rel_c1, G.rel_c2, G.sw_c1, G.sw_c2, G.reg_node) == G.matrix_free
    deg = np.bincount(np.concatenate([G.rel_c1, G.rel_c2, G.sw_c1, G.sw_c2]), minlength=G.n_poses)
    if not G.matrix_free:
        assert deg.max() == 257 or np.bincount(G.reg_node).max() == 2      # just past the limit: one side too many, or a second regulariser
        return
    nr.tile_invariants(T, G.n_poses)
    assert nr.tile_condition(T, G.condition), (T["lanes"], np.diff(T["node0"]))
    if name.startswith("hub256"):
        assert deg.max() == 256 and deg[137] == 256
        t = int(np.searchsorted(T["node0"], 137, side="right") - 1)
        assert T["node0"][t] == 137 and T["node0"][t + 1] == 138 and T["lanes"][t] == 256      # alone in its tile
    if name == "hub256-parallel":
        pairs = set(zip(G.rel_c1.tolist(), G.rel_c2.tolist()))
        assert sum(1 for (a, b) in pairs if a == 137 and (b, a) in pairs) >= 127
    if name.startswith("lanes"):
        assert T["closed_by"].count("lanes") >= 3
    if name == "gap":
        t = int(np.flatnonzero(T["lanes"] == 0)[0])
        assert T["sides"][t] == 0 and 0 < T["lanes"][t - 1] < 42 and 0 < T["lanes"][t + 1] < 42      # a whole tile without sides between two half-empty ones
    if name.startswith("boundary"):
        assert T["node0"][1] == 42      # the pairs (41, 42) / (42, 41) straddle the first boundary


def test_the_big_graph_makes_some_workgroups_take_two_trips():
    G = nc.big_graph()
    T = nr.tile_rule(G.n_poses, G.rel_c1, G.rel_c2, G.sw_c1, G.sw_c2)
    nr.tile_invariants(T, G.n_poses)
    assert T["n_tiles"] > nr.MF_MAX_GRID and T["n_tiles"] % nr.MF_MAX_GRID != 0


# name -> (case, variant)
TEETH = {
    "one side of an in-tile pair dropped": ("lanes-rel", ("drop_side", 10, 0)),                 # chain edge (11, 10): both keyframes in the first tile
    "two parallel edges exchange a block": ("boundary43", ("swap_parallel", 42, 44)),          # the two extra (41, 42) edges: rel slots 42 and 44 after the 42 chain edges
    "a switch's rank-one term omitted":    ("lanes-sw", ("omit_switch", 5)),
    "no damping on one keyframe":          ("hub256", ("no_damping", 137)),
    "a c1 > c2 edge transposed":           ("lanes-rel", ("transpose", 300)),                   # the second loop, entered as (far, near): the coupling block of a long edge is far from symmetric
}


@pytest.mark.parametrize("radius", nc.RADII)
@pytest.mark.parametrize("tooth", sorted(TEETH))
def test_wrong_variants_show_in_the_gpu_tests_comparison(tooth, radius):
    name, variant = TEETH[tooth]
    G = nc.graph(name)
    if variant[0] == "swap_parallel":
        e1, e2 = variant[1], variant[2]
        assert (G.rel_c1[e1], G.rel_c2[e1]) == (G.rel_c1[e2], G.rel_c2[e2]) == (41, 42)
    if variant[0] == "transpose":
        assert G.rel_c1[variant[1]] > G.rel_c2[variant[1]]
    if variant[0] == "drop_side":
        T = nr.tile_rule(G.n_poses, G.rel_c1, G.rel_c2, G.sw_c1, G.sw_c2)
        assert G.rel_c1[variant[1]] < T["node0"][1] and G.rel_c2[variant[1]] < T["node0"][1]
    ref = nc.reference(name, radius)
    q, t, s = nc.state(G)
    wrong = nr.reference(nc.oracle_problem(G), G, q, t, s, radius, variant=variant)
    good = nr.compare(ref.A.toarray(), ref.A.toarray())
    bad = nr.compare(wrong.A.toarray(), ref.A.toarray())
    print("NORMALOP tooth %-38s radius %.0e  err %.3e  err_block %.3e" % (tooth, radius, bad["err"], bad["err_block"]))
    assert good["worst"] == 0.0 and good["nonzero_outside"] == 0
    assert bad["worst"] >= 1e-6


def test_comparison_sees_a_stray_block_and_a_small_block_next_to_a_hub():
    ref = nc.reference("hub256", nc.RADII[0]).A.toarray()
    stray = ref.copy()
    stray[6 * 3, 6 * 250] = 1e-300      # keyframes 3 and 250 share no edge
    assert nr.compare(stray, ref)["nonzero_outside"] == 1
    # a relative error of 1e-6 in the coupling of two low-degree keyframes: invisible in the max-norm under the hub's diagonal, visible in the block measure
    small = ref.copy()
    small[6 * 11:6 * 11 + 6, 6 * 10:6 * 10 + 6] *= 1.0 + 1e-6
    c = nr.compare(small, ref)
    assert c["err"] < 1e-10 < 1e-9 <= c["err_block"]      # (the GPU test's tolerance lies between the two)


def test_sparse_pcg_equals_the_dense_model():
    from tests import precond_model as pm
    G = nc.graph("gap")
    ref = nc.reference("gap", nc.RADII[0])
    A, b, free = nr.device_rows(ref, G.constant)
    x = nr.pcg(A, b, nr.block_jacobi_factors(nr.diagonal_blocks(A)), 3)
    rows = np.flatnonzero(np.repeat(free, 6))
    Ad = A.toarray()[np.ix_(rows, rows)]
    xd = pm.pcg(Ad, b[rows], pm.block_jacobi(Ad), 3)
    x32 = nr.pcg(A, b, nr.block_jacobi_factors(nr.diagonal_blocks(A), fp32=True), 3)
    xd32 = pm.pcg(Ad, b[rows], pm.block_jacobi(Ad, fp32=True), 3)
    for k in range(3):
        assert np.abs(x[k][rows] - xd[k]).max() <= 1e-12 * np.abs(xd[k]).max() and np.all(x[k][~np.repeat(free, 6)] == 0.0)
        assert np.abs(x32[k][rows] - xd32[k]).max() <= 1e-12 * np.abs(xd32[k]).max()
