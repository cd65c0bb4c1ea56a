"""CPU: the host side of the tile-sparse Cholesky solver (csrc/pgo_sparse_math.hpp: the orderings, the tile pattern, the symbolic factorisation, the order of the block
steps and the serial instantiation of the factor and the solve) through tests/native/sparse_chol_host.cpp, against numpy.  The header is host-only so far: no kernel and
no option of the library uses it yet.

Symbolic: the plan's pattern of L against a brute-force boolean Cholesky of the tile matrix (for every column k, every pair of its non-zero rows is non-zero), the tile
matrix of a graph formed here from the edge list, independently of the header.

Numeric: in natural order every tile operation the sparse factorisation skips would have produced or subtracted a zero in the dense one, so the sparse solve equals
dc_host_solve AS NUMBERS (np.array_equal; the sign of a zero may differ).  Under a permutation it is another rounding of the same solution: eta <= n u, the bound and eta
of tests/test_dense_cholesky_host.py, which derives the bound."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from solve_keyframe_pose_graph_amd import graphgen
from tests import precond_cases as pc
from tests.test_dense_cholesky_host import U, eta

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "solve_keyframe_pose_graph_amd", "csrc")
SRC = os.path.join(HERE, "native", "sparse_chol_host.cpp")
NB = 64
ORDER_AUTO, ORDER_NATURAL, ORDER_RCM = -1, 0, 1      # sc_plan_graph's `ordering`
# what the shim reports of a plan
INFO = ("nt", "a_tiles", "l_tiles", "ordering", "bytes", "factor_launches", "solve_launches", "tile_updates")


def ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t)) if a is not None else None


@pytest.fixture(scope="module")
def shim():
    so = os.path.join(HERE, "native", "libsparse_chol_host.so")
    hdrs = [os.path.join(CSRC, h) for h in ("pgo_sparse_math.hpp", "pgo_dense_math.hpp")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [SRC] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, "-o", so, SRC])
    lib = C.CDLL(so)
    lib.sch_symbolic.restype = C.c_int64
    lib.sch_graph_plan.restype = C.c_int64
    return lib


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# symbolic
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def boolean_cholesky(A):
    """the pattern of L of a symmetric boolean tile matrix (lower triangle, diagonal set): no cancellation"""
    L = np.tril(A).astype(bool)
    nt = len(L)
    for k in range(nt):
        rows = np.nonzero(L[k + 1:, k])[0] + k + 1
        for j in rows:
            L[rows[rows >= j], j] = True
    return L


def symbolic(shim, A):
    nt = len(A)
    ti, tj = np.nonzero(np.tril(A, -1))
    ti, tj = np.ascontiguousarray(ti, dtype=np.int32), np.ascontiguousarray(tj, dtype=np.int32)
    by_row, by_col, info = np.zeros((nt, nt), np.uint8), np.zeros((nt, nt), np.uint8), np.zeros(8, np.int64)
    bad = shim.sch_symbolic(C.c_int(nt), C.c_int64(len(ti)), ptr(ti, C.c_int32), ptr(tj, C.c_int32), ptr(by_row, C.c_uint8), ptr(by_col, C.c_uint8), ptr(info, C.c_int64))
    return bad, by_row.astype(bool), by_col.astype(bool), dict(zip(INFO, [int(v) for v in info]))


def check_info(info, A, L):
    nt = len(L)
    s = [int(L[k + 1:, k].sum()) for k in range(nt)]
    assert info["nt"] == nt and info["a_tiles"] == int(np.tril(A).astype(bool).sum()) and info["l_tiles"] == int(L.sum()) and info["bytes"] == int(L.sum()) * 4096 * 8
    assert info["tile_updates"] == sum(m * (m + 1) // 2 for m in s) and info["solve_launches"] == 2 * nt
    # the steps a launcher would launch: one for the first diagonal tile; a step with a non-empty s_k: panel + update, and one more where tile k + 1 is not in s_k; an empty s_k: the next diagonal tile alone
    assert info["factor_launches"] == 1 + sum((2 if L[k + 1, k] else 3) if s[k] else 1 for k in range(nt - 1))


@pytest.mark.parametrize("seed", range(12))
def test_symbolic_factorisation_of_random_tile_patterns(shim, seed):
    rng = np.random.default_rng(seed)
    nt = int(rng.integers(1, 41))
    A = rng.random((nt, nt)) < rng.choice([0.02, 0.08, 0.3])
    A = A | A.T | np.eye(nt, dtype=bool)
    bad, by_row, by_col, info = symbolic(shim, A)
    L = boolean_cholesky(A)
    assert bad == 0      # every (a >= b) pair of every s_k resolves to a tile, tile ids agree between the two lists
    assert np.array_equal(by_row, L) and np.array_equal(by_col, L)
    check_info(info, A, L)


def adjacency(g, constant=()):
    """(adj_ptr, adj, in_system) over all edges of the graph: what the solver reads of its block-CSR structure (the keyframe itself first, duplicates kept)"""
    N = g.n_poses
    c1 = np.concatenate([g.odom_c1, g.loop_c1]).astype(np.int64); c2 = np.concatenate([g.odom_c2, g.loop_c2]).astype(np.int64)
    nb = [[i] for i in range(N)]
    for a, b in zip(c1, c2):
        nb[a].append(int(b)); nb[b].append(int(a))
    adj_ptr = np.zeros(N + 1, np.int64); adj_ptr[1:] = np.cumsum([len(v) for v in nb])
    adj = np.ascontiguousarray(np.concatenate(nb), dtype=np.int32)
    in_system = np.zeros(N, np.uint8)
    in_system[np.unique(np.concatenate([c1, c2, np.asarray(g.reg_node, dtype=np.int64)]))] = 1
    in_system[list(constant)] = 0
    return adj_ptr, adj, in_system, c1, c2


def graph_plan(shim, g, ordering, constant=()):
    adj_ptr, adj, in_system, c1, c2 = adjacency(g, constant)
    N = g.n_poses
    nt = shim.sch_nt_of(C.c_int64(N))
    order, by_row, by_col, info = np.zeros(N, np.int32), np.zeros((nt, nt), np.uint8), np.zeros((nt, nt), np.uint8), np.zeros(8, np.int64)
    bad = shim.sch_graph_plan(C.c_int64(N), ptr(adj_ptr, C.c_int64), ptr(adj, C.c_int32), ptr(in_system, C.c_uint8), C.c_int(ordering), ptr(order, C.c_int32), ptr(by_row, C.c_uint8),
                              ptr(by_col, C.c_uint8), ptr(info, C.c_int64))
    return bad, order, by_row.astype(bool), by_col.astype(bool), dict(zip(INFO, [int(v) for v in info])), (in_system, c1, c2, nt)


def tile_matrix(N, order, in_system, c1, c2, nt):
    """the tile pattern of the system with keyframe order[q] at position q, formed from the scalar entries: six rows per keyframe, which may straddle two tiles"""
    pos = np.empty(N, np.int64); pos[order] = np.arange(N)
    A = np.eye(nt, dtype=bool)
    k6 = np.arange(6)
    keep = (in_system[c1] != 0) & (in_system[c2] != 0)
    nodes = np.nonzero(in_system)[0]
    for a, b in zip(np.concatenate([c1[keep], nodes]), np.concatenate([c2[keep], nodes])):
        hi, lo = (a, b) if pos[a] >= pos[b] else (b, a)
        r, c = np.meshgrid(6 * pos[hi] + k6, 6 * pos[lo] + k6, indexing="ij")
        m = c <= r
        A[r[m] // NB, c[m] // NB] = True
    return A | A.T


GRAPHS = {"tl200": lambda: pc.graph("tl200"), "tl600": lambda: pc.graph("tl600"), "g1100": lambda: graphgen.generate(1100, 110, odom_f_max=5, seed=7)}


@pytest.mark.parametrize("ordering", [ORDER_NATURAL, ORDER_RCM])
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_symbolic_factorisation_of_graph_tile_patterns(shim, name, ordering):
    g = GRAPHS[name]()
    bad, order, by_row, by_col, info, (in_system, c1, c2, nt) = graph_plan(shim, g, ordering)
    assert bad == 0 and info["ordering"] == ordering
    assert np.array_equal(np.sort(order), np.arange(g.n_poses))
    A = tile_matrix(g.n_poses, order, in_system, c1, c2, nt)
    L = boolean_cholesky(A)
    assert np.array_equal(by_row, L) and np.array_equal(by_col, L)
    check_info(info, A, L)
    print("SPARSE host plan %s ordering %d: nt %d, tiles of the matrix %d, of L %d (dense %d), launches %d + %d, tile updates %d"
          % (name, ordering, info["nt"], info["a_tiles"], info["l_tiles"], nt * (nt + 1) // 2, info["factor_launches"], info["solve_launches"], info["tile_updates"]))


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# ordering
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_rcm_is_a_deterministic_permutation_with_the_outsiders_last(shim):
    g = pc.graph("tl600", 3)      # the last three keyframes are referenced by nothing
    constant = pc.CONSTANT_TL600
    outs = []
    for _ in range(2):
        bad, order, _, _, info, (in_system, _, _, _) = graph_plan(shim, g, ORDER_RCM, constant)
        assert bad == 0 and info["ordering"] == 1
        outs.append(order)
    assert np.array_equal(outs[0], outs[1])
    assert np.array_equal(np.sort(outs[0]), np.arange(g.n_poses))
    outside = np.nonzero(in_system == 0)[0]
    assert len(outside) == len(constant) + 3
    assert np.array_equal(outs[0][-len(outside):], outside)      # by index, after every keyframe of the system
    _, natural, _, _, _, _ = graph_plan(shim, g, ORDER_NATURAL, constant)
    assert np.array_equal(natural, np.arange(g.n_poses))


def test_rcm_starts_every_component_at_its_lowest_degree_keyframe(shim):
    """two chains 0-1-2-3 and 4-5-6 with a pendant 7 on keyframe 5: Cuthill-McKee starts at keyframe 0 (degree 1, lowest index), numbers 0 1 2 3, then the second
    component from keyframe 4 (degree 1): 4, 5, then 5's neighbours by (degree, index): 6, 7; reversed"""
    class G:
        n_poses = 8
        odom_c1, odom_c2 = np.array([0, 1, 2, 4, 5, 5]), np.array([1, 2, 3, 5, 6, 7])
        loop_c1 = loop_c2 = np.zeros(0, np.int64)
        reg_node = np.zeros(0, np.int64)
    _, order, _, _, _, _ = graph_plan(shim, G, ORDER_RCM)
    assert list(order) == [7, 6, 5, 4, 3, 2, 1, 0]


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_auto_keeps_the_order_with_fewer_tiles(shim, name):
    g = GRAPHS[name]()
    tiles = {o: graph_plan(shim, g, o)[4] for o in (ORDER_AUTO, ORDER_NATURAL, ORDER_RCM)}
    auto, nat, rcm = (tiles[o] for o in (ORDER_AUTO, ORDER_NATURAL, ORDER_RCM))
    assert auto["l_tiles"] == min(nat["l_tiles"], rcm["l_tiles"])
    assert auto["ordering"] == (1 if rcm["l_tiles"] < nat["l_tiles"] else 0)      # natural wins a tie


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# numeric
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def patterned(n, tiles, seed):
    """a symmetric positive definite matrix whose non-zeros are the diagonal tiles and `tiles` (tile row > tile column), cut at n: random entries, then a stiff low-rank
    part inside every diagonal tile and a small damping — the conditioning of tests/test_dense_cholesky_host.py's matrices without their fill"""
    rng = np.random.default_rng(seed)
    nt = (n + NB - 1) // NB
    mask = np.zeros((nt * NB, nt * NB), bool)
    for t in range(nt):
        mask[t * NB:(t + 1) * NB, t * NB:(t + 1) * NB] = True
    for i, j in tiles:
        mask[i * NB:(i + 1) * NB, j * NB:(j + 1) * NB] = True
    mask = (mask | mask.T)[:n, :n]
    B = rng.standard_normal((n, n)) * mask
    A = 0.5 * (B + B.T)
    A = A + np.diag(np.abs(A).sum(axis=1) * rng.uniform(1.0, 1.0 + 1e-3, n) + rng.uniform(1e-3, 1.0, n))
    return A, rng.standard_normal(n)


def full(n):
    from tests.test_dense_cholesky_host import spd
    return spd(n)


# name -> (n, the off-diagonal tiles, the tiles of L expected); n <= 448
CASES = {
    "one_tile": (64, [], 1),
    "padding": (96, [(1, 0)], 3),
    "block_diagonal": (128, [], 2),                                          # s_0 is empty: the diagonal tile of step 1 is a step of its own
    "arrow": (320, [(4, 0), (4, 1), (4, 2), (4, 3)], 9),                      # fill only inside the last tile row
    "fill_only_tile": (192, [(1, 0), (2, 0)], 6),                             # tile (2, 1) exists only as fill
    "band": (448, [(k + 1, k) for k in range(6)], 13),
    "band_odd": (400, [(k + 1, k) for k in range(6)] + [(k + 2, k) for k in range(5)], 18),
}


def solve(shim, A, b, pos=None):
    A = np.ascontiguousarray(A); b = np.ascontiguousarray(b)
    x, info = np.full(len(b), 7.0), np.zeros(8, np.int64)
    p = None if pos is None else np.ascontiguousarray(pos, dtype=np.int32)
    ok = shim.sch_solve(C.c_int(len(b)), ptr(A, C.c_double), ptr(b, C.c_double), ptr(p, C.c_int32), ptr(x, C.c_double), ptr(info, C.c_int64))
    return bool(ok), x, dict(zip(INFO, [int(v) for v in info]))


def dense_solve(shim, A, b):
    A = np.ascontiguousarray(A); b = np.ascontiguousarray(b)
    x = np.full(len(b), 7.0)
    assert shim.sch_dense_solve(C.c_int(len(b)), ptr(A, C.c_double), ptr(b, C.c_double), ptr(x, C.c_double)) == 1
    return x


@pytest.mark.parametrize("name", sorted(CASES))
def test_natural_order_equals_the_dense_host_solve_as_numbers(shim, name):
    n, tiles, l_tiles = CASES[name]
    A, b = patterned(n, tiles, n)
    ok, x, info = solve(shim, A, b)
    assert ok and info["l_tiles"] == l_tiles and info["a_tiles"] == len(tiles) + (n + NB - 1) // NB
    xd = dense_solve(shim, A, b)
    e = eta(A, b, x)
    print("SPARSE host %s n %d  tiles of L %d  eta %.3e = %.2f u (bound n u = %.3e)" % (name, n, info["l_tiles"], e, e / U, n * U))
    assert np.array_equal(x, xd)
    assert e <= n * U


@pytest.mark.parametrize("n", [64, 200, 448])
def test_a_full_matrix_equals_the_dense_host_solve_as_numbers(shim, n):
    A, b = full(n)
    ok, x, info = solve(shim, A, b)
    nt = (n + NB - 1) // NB
    assert ok and info["l_tiles"] == nt * (nt + 1) // 2 and info["factor_launches"] == 1 + 2 * (nt - 1)      # the dense solver's step count
    assert np.array_equal(x, dense_solve(shim, A, b))
    assert eta(A, b, x) <= n * U


@pytest.mark.parametrize("name", ["arrow", "band", "fill_only_tile", "full"])
def test_a_permutation_of_the_nodes_is_solved_to_the_bound(shim, name):
    if name == "full":
        n = 444
        A, b = full(n)
    else:
        n, tiles, _ = CASES[name]
        n = n // 6 * 6      # whole 6-row nodes
        A, b = patterned(n, tiles, n + 1)
    rng = np.random.default_rng(5)
    node_pos = rng.permutation(n // 6)
    pos = (6 * node_pos[:, None] + np.arange(6)[None, :]).reshape(-1)
    ok, x, info = solve(shim, A, b, pos)
    assert ok
    e = eta(A, b, x)
    print("SPARSE host %s permuted n %d  tiles of L %d  eta %.3e = %.2f u (bound n u = %.3e)" % (name, n, info["l_tiles"], e, e / U, n * U))
    assert e <= n * U


def test_an_indefinite_matrix_a_nan_and_a_zero_pivot_are_reported_not_factored(shim):
    A = np.eye(128); A[70, 70] = -1.0
    ok, x, _ = solve(shim, A, np.ones(128))
    assert not ok and np.all(x == 7.0)
    A = np.eye(128); A[100, 3] = A[3, 100] = np.nan
    ok, x, _ = solve(shim, A, np.ones(128))
    assert not ok and np.all(x == 7.0)
    A = np.eye(64); A[63, 63] = 0.0      # a zero pivot is not > 0 either
    ok, x, _ = solve(shim, A, np.ones(64))
    assert not ok and np.all(x == 7.0)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# the same code in a sanitized stand-alone program
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_stand_alone_program_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "sparse_chol_host_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DSCH_MAIN", "-I", CSRC, "-o", exe, SRC])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-2000:] + out.stderr[-2000:]
