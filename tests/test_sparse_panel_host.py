"""CPU: the host side of the columns of the inverse in number (csrc/pgo_sparse_math.hpp: sc_panel_steps, ScPanelHost, ScPlan::panel_launches / panel_products;
csrc/pgo_sparse_blocks.hpp: sc_column_chunks, ScColumns and the gather) through tests/native/sparse_panel_host.cpp, and sparse_cholesky.cross_blocks /
gate_from_blocks — the host-testable halves of cross_covariance and loop_candidate_gate — on top of it.  The kernels run on the GPU only
(tests/test_gpu_sparse_panel.py, which takes its matrices, references and the host instantiation from here).

Reference and error measure: tests/test_sparse_selinv_host.py's — the refined inverse (np.longdouble Newton steps) of the eleven matrices and the three permuted ones,
the scaled entrywise e — here over ALL entries: every column of the inverse is solved, none is outside a pattern.  Bound: MARGIN x e_np, e_np being plain fp64 numpy
(Cholesky factor, triangular inverse, Gram product) on the same matrix; the panel sweeps are the same backward-stable factor followed by two triangular substitutions.
Two paths of the library against each other (panel sweeps and the two sweeps of ScHost on the same unit columns) are held to twice that: the sum of their bounds.
Every test prints its figures (`SPARSE panel ...`) before it asserts."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
import scipy.linalg

from solve_keyframe_pose_graph_amd import _build
from solve_keyframe_pose_graph_amd import sparse_cholesky as sc
from tests import dense_cov_ref as dref
from tests import param_cov_ref as pref
from tests.test_sparse_cholesky_host import boolean_cholesky
from tests.test_sparse_companion_host import block_system, host_reduce
from tests.test_sparse_companion_host import load_shim as load_companion_shim
from tests.test_sparse_selinv_host import CONSTANT_24, GATHER_N, NAMES, PERMUTED, full_matrix_of, gauss_newton_case, matrix, permuted_matrix, reference

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "solve_keyframe_pose_graph_amd", "csrc")
SRC = os.path.join(HERE, "native", "sparse_panel_host.cpp")
HEADERS = ("pgo_sparse_blocks.hpp", "pgo_sparse_math.hpp", "pgo_dense_math.hpp")
NB = 64
MARGIN = dref.MARGIN
dp, ip, lp, bp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_longlong), C.POINTER(C.c_ubyte)
I32 = lambda x: np.ascontiguousarray(x, dtype=np.int32)
F64 = lambda x: np.ascontiguousarray(x, dtype=np.float64)


def load_shim():
    so = os.path.join(HERE, "native", "libsparse_panel_host.so")
    deps = [SRC] + [os.path.join(CSRC, h) for h in HEADERS]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, "-o", so, SRC])
    lib = C.CDLL(so)
    lib.spp_plan_counts.restype = C.c_longlong
    lib.spp_plan_counts.argtypes = [C.c_int, C.c_longlong, ip, ip, C.c_int, ip, C.c_int, lp, ip]
    lib.spp_chunks.restype = C.c_longlong
    lib.spp_chunks.argtypes = [C.c_longlong, C.c_int, C.c_longlong, lp]
    lib.spp_matrix.argtypes = [C.c_int, dp, ip, C.c_int, ip, C.c_int, dp, dp, lp]
    lib.spp_create.restype = C.c_void_p
    lib.spp_create.argtypes = [C.c_longlong, bp, C.c_longlong, ip, ip, C.c_int]
    lib.spp_destroy.argtypes = [C.c_void_p]
    lib.spp_info.argtypes = [C.c_void_p, ip]
    lib.spp_factor.argtypes = [C.c_void_p, dp, dp]
    lib.spp_inverse_columns.argtypes = [C.c_void_p, C.c_longlong, ip, C.c_longlong, ip, ip, C.c_longlong, dp, lp]
    lib.spp_solve.argtypes = [C.c_void_p, C.c_longlong, dp, dp]
    return lib


@pytest.fixture(scope="module")
def shim():
    return load_shim()


def same_bits(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.shape == y.shape and x.tobytes() == y.tobytes()


def scaled(X, S_ref):
    """dense_cov_ref's scaled entrywise error of X against the (longdouble) reference"""
    d = np.sqrt(np.diag(S_ref).astype(np.float64))
    return float((np.abs(X.astype(np.longdouble) - S_ref).astype(np.float64) / np.outer(d, d)).max())


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# the panel sweeps through the matrix interface's plan
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def host_columns(shim, A, cols, pos=None, k_stop=0, sweeps=False):
    """(X [len(cols)][n]: the columns `cols` of the inverse by the panel sweeps, the same by ScHost's two sweeps or None, launches, tile products)"""
    A, cols = F64(A), I32(cols)
    n = len(A)
    X, Xs, info = np.full((len(cols), n), 7.0), (np.full((len(cols), n), 7.0) if sweeps else None), np.zeros(2, np.int64)
    p = None if pos is None else I32(pos)
    rc = shim.spp_matrix(n, A.ctypes.data_as(dp), None if p is None else p.ctypes.data_as(ip), len(cols), cols.ctypes.data_as(ip), k_stop, X.ctypes.data_as(dp),
                         None if Xs is None else Xs.ctypes.data_as(dp), info.ctypes.data_as(lp))
    assert rc == 1
    return X, Xs, int(info[0]), int(info[1])


@functools.lru_cache(maxsize=None)
def all_columns(name, permuted=False):
    """the whole inverse by the panel sweeps and by ScHost's two sweeps: computed once, read-only"""
    A = reference(name, permuted)[0]
    pos = permuted_matrix(name)[1] if permuted else None
    X, Xs, launches, products = host_columns(load_shim(), A, np.arange(len(A)), pos, sweeps=True)
    X.setflags(write=False); Xs.setflags(write=False)
    return X, Xs, launches, products


def check_whole_inverse(tag, name, permuted):
    A, S_ref, S_np = reference(name, permuted)
    n = len(A)
    X, Xs, launches, products = all_columns(name, permuted)
    e, e_np, between = scaled(X, S_ref), scaled(S_np, S_ref), scaled(X, Xs.astype(np.longdouble))
    print("SPARSE panel host %-24s n %3d  panels %d  launches %2d  products %3d  e %.3e  e_np %.3e  e / e_np %.2f  against the two sweeps %.3e  (bounds %g e_np, %g e_np)"
          % (tag, n, (n + NB - 1) // NB, launches, products, e, e_np, e / e_np, between, MARGIN, 2 * MARGIN))
    nt = (n + NB - 1) // NB
    assert launches == 2 * nt      # every column: the first panel starts in tile 0, the lowest requested row is in tile 0
    assert e <= MARGIN * e_np
    assert between <= 2.0 * MARGIN * e_np


@pytest.mark.parametrize("name", NAMES)
def test_panel_sweeps_over_all_columns_against_the_refined_inverse(name):
    check_whole_inverse(name, name, False)


@pytest.mark.parametrize("name", PERMUTED)
def test_panel_sweeps_under_a_permutation_of_the_nodes(name):
    check_whole_inverse(name + " permuted", name, True)


EDGE = "full448"      # nt = 7, 74 whole nodes: every tile stored, so every panel and sweep edge below has products to go wrong in


@pytest.mark.parametrize("tag, nodes, k_stop, panels", [
    ("11 keyframes: 66 rows, two panels, node 10 straddles them", range(11), 0, 2),
    ("32 keyframes: exactly three full panels", range(32), 0, 3),
    ("one keyframe: a quarter of a wavefront's rows", [10], 0, 1),
    ("columns only late: first > 0", range(40, 74), 0, 4),
    ("rows only late: k_stop > 0", range(0, 74, 3), 4, 3),
    ("late columns and late rows", range(50, 74), 5, 3),
])
def test_panel_and_sweep_edges_give_the_bits_of_the_whole_inverse(shim, tag, nodes, k_stop, panels):
    A, S_ref, S_np = reference(EDGE)
    n, nt = len(A), len(A) // NB
    cols = dref.node_columns(list(nodes))
    X, _, launches, products = host_columns(shim, A, cols[::-1].copy(), k_stop=k_stop)      # (given in descending order: the layout sorts them by position)
    X = X[::-1]
    whole = all_columns(EDGE)[0]
    first = [int(cols[p * NB]) // NB for p in range(panels)]
    live = slice(NB * k_stop, n)      # the entries the backward sweep reached
    d = np.sqrt(np.diag(S_ref).astype(np.float64))
    rows_error = lambda Y: float((np.abs(Y.astype(np.longdouble) - S_ref[cols]).astype(np.float64) / np.outer(d[cols], d))[:, live].max())
    e, e_np = rows_error(X), rows_error(S_np[cols])
    print("SPARSE panel edges %-58s rows %3d  panels %d  first %s  k_stop %d  launches %2d  products %3d  e %.3e  e_np %.3e  equal bits with the whole inverse: %s"
          % (tag, len(cols), panels, first, k_stop, launches, products, e, e_np, same_bits(X[:, live], whole[cols][:, live])))
    assert (len(cols) + NB - 1) // NB == panels == len(first)
    assert launches == (nt - first[0]) + (nt - k_stop)
    # a full matrix stores every tile (k, j), j < k: forward, panel p multiplies k - first[p] tiles in step k; backward, nt - 1 - k tiles per panel in step k
    assert products == sum(k - f for f in first for k in range(f, nt)) + panels * sum(nt - 1 - k for k in range(k_stop, nt))
    assert same_bits(X[:, live], whole[cols][:, live])      # alone, in another batch, with other panels and another k_stop: the same bits
    assert e <= MARGIN * e_np


def test_one_tile_and_an_empty_column(shim):
    """nt = 1: one step per sweep and no product; `gap`: s_1 and s_3 are empty, the backward step of such a column is the substitution alone"""
    A = reference("full64")[0]
    X, _, launches, products = host_columns(shim, A, np.arange(64))
    assert launches == 2 and products == 0 and same_bits(X, all_columns("full64")[0])
    A = matrix("gap")
    L = boolean_cholesky(np.abs(A.reshape(5, NB, 5, NB)).max(axis=(1, 3)) > 0)
    s = [int(L[k + 1:, k].sum()) for k in range(5)]
    X, _, launches, products = host_columns(shim, A, np.arange(NB, 2 * NB))      # the columns of tile 1: first = 1
    print("SPARSE panel gap: s_k sizes %s  launches %d  products %d" % (s, launches, products))
    assert s[1] == 0 and s[3] == 0 and launches == 4 + 5
    assert products == sum(int(L[k, 1:k].sum()) for k in range(1, 5)) + sum(s)
    assert same_bits(X, all_columns("gap")[0][NB:2 * NB])


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# the counts and the order of the steps
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(8))
def test_counts_and_step_order_on_random_tile_patterns(shim, seed):
    rng = np.random.default_rng(100 + seed)
    nt = int(rng.integers(1, 41))
    A = rng.random((nt, nt)) < rng.choice([0.02, 0.08, 0.3])
    A = A | A.T | np.eye(nt, dtype=bool)
    n_panels = int(rng.integers(1, 7))
    first = np.sort(rng.integers(0, nt, n_panels)).astype(np.int32)
    k_stop = int(rng.integers(0, nt))
    ti, tj = np.nonzero(np.tril(A, -1))
    ti, tj = I32(ti), I32(tj)
    counts, trace = np.zeros(2, np.int64), np.zeros(6 * nt, np.int32)
    calls = shim.spp_plan_counts(nt, len(ti), ti.ctypes.data_as(ip), tj.ctypes.data_as(ip), n_panels, first.ctypes.data_as(ip), k_stop, counts.ctypes.data_as(lp), trace.ctypes.data_as(ip))
    L = boolean_cholesky(A)
    forward = sum(int(L[k, f:k].sum()) for f in first for k in range(int(f), nt))
    backward = n_panels * sum(int(L[k + 1:, k].sum()) for k in range(k_stop, nt))
    print("SPARSE panel plan seed %d: nt %2d  tiles of L %3d  panels %d  first %s  k_stop %2d  launches %3d  products %4d (forward %d, backward %d)"
          % (seed, nt, int(L.sum()), n_panels, [int(f) for f in first], k_stop, int(counts[0]), int(counts[1]), forward, backward))
    want = [(0, k, int((first <= k).sum())) for k in range(int(first[0]), nt)] + [(1, k, n_panels) for k in range(nt - 1, k_stop - 1, -1)]
    assert [tuple(r) for r in trace[:3 * calls].reshape(-1, 3)] == want      # forward from the first started tile over the started prefix, then backward over all panels down to k_stop
    assert int(counts[0]) == len(want) == calls and int(counts[1]) == forward + backward


def test_chunks_lie_on_whole_keyframes_and_fit_the_limit(shim):
    for n_cols, nc, limit in ((38, 256, 64 * 256 * 8), (1000, 6656, 1 << 30), (25, 256, 3 * 64 * 256 * 8), (7, 64, 64 * 64 * 8 - 1)):
        bounds = np.zeros(2 * n_cols, np.int64)
        runs = shim.spp_chunks(n_cols, nc, limit, bounds.ctypes.data_as(lp))
        b = bounds[:2 * runs].reshape(-1, 2)
        print("SPARSE panel chunks: %4d column keyframes  nc %4d  limit %10d  runs %s" % (n_cols, nc, limit, [(int(x), int(y)) for x, y in b][:6]))
        if limit < 64 * nc * 8:
            assert runs == 0      # below one panel
            continue
        assert b[0, 0] == 0 and b[-1, 1] == n_cols and np.array_equal(b[1:, 0], b[:-1, 1]) and np.all(b[:, 1] > b[:, 0])
        assert all((6 * (e - s) + NB - 1) // NB * NB * nc * 8 <= limit for s, e in b)
        assert all(6 * (e - s + 1) > limit // (NB * nc * 8) * NB for s, e in b[:-1])      # a run takes what fits


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# the block interface on the host
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
class HostColumns:
    """the shim's pgo_sparse_chol_{create, factor, inverse_columns, columns_info, set_workspace_limit, solve}: SparseCholesky's methods of the same names"""

    def __init__(self, lib, N, in_system, hi, lo, ordering):
        self.lib, self.N = lib, N
        self.ins, self.hi, self.lo = np.ascontiguousarray(in_system, dtype=np.uint8), I32(hi), I32(lo)
        self.h = lib.spp_create(N, self.ins.ctypes.data_as(bp), len(self.hi), self.hi.ctypes.data_as(ip), self.lo.ctypes.data_as(ip), ordering)
        self.limit, self.info4, self.rc, self.n_nodes = sc.WORKSPACE_BYTES, np.zeros(4, np.int64), 0, N

    def last_ms(self):
        return 0.0      # (no device, no events)

    def nt(self):
        return self.lib.spp_info(self.h, None)

    def order(self):
        order = np.zeros(self.N, np.int32)
        self.lib.spp_info(self.h, order.ctypes.data_as(ip))
        return order

    def factor(self, diag, blocks):
        d, b = F64(diag), F64(blocks)
        return self.lib.spp_factor(self.h, d.ctypes.data_as(dp), b.ctypes.data_as(dp)) == 1

    def set_workspace_limit(self, nbytes):
        self.limit = int(nbytes)

    def inverse_columns(self, col_nodes, row_nodes, col_index, fill=0.0):
        cn, rn, ci = I32(col_nodes).reshape(-1), I32(row_nodes).reshape(-1), I32(col_index).reshape(-1)
        out = np.full((len(rn), 6, 6), fill)
        self.rc = self.lib.spp_inverse_columns(self.h, len(cn), cn.ctypes.data_as(ip), len(rn), rn.ctypes.data_as(ip), ci.ctypes.data_as(ip), self.limit, out.ctypes.data_as(dp), self.info4.ctypes.data_as(lp))
        return out

    def columns_info(self):
        return dict(zip(sc.COLUMNS_INFO, [int(v) for v in self.info4]))

    def solve(self, B):
        B = F64(B).reshape(-1, 6 * self.N)
        X = np.full_like(B, 7.0)
        self.lib.spp_solve(self.h, len(B), B.ctypes.data_as(dp), X.ctypes.data_as(dp))
        return X

    def close(self):
        if self.h:
            self.lib.spp_destroy(self.h)
            self.h = None


def as_block_system(A):
    """(N, hi, lo, diag, blocks): the n x n matrix as 6 x 6 blocks, padded by identity rows to N = ceil(n / 6) whole blocks; a pair per non-zero off-diagonal block
    (tests/test_gpu_sparse_selinv.py's)"""
    n = len(A)
    N = (n + 5) // 6
    B = np.eye(6 * N); B[:n, :n] = A
    T = B.reshape(N, 6, N, 6).transpose(0, 2, 1, 3)
    nz = np.abs(T).max(axis=(2, 3)) > 0
    hi, lo = np.nonzero(np.tril(nz, -1))
    return N, hi.astype(np.int32), lo.astype(np.int32), np.ascontiguousarray(T[np.arange(N), np.arange(N)]), np.ascontiguousarray(T[hi, lo])


def whole_inverse_blocks(F, N):
    """every block of the inverse through inverse_columns, all keyframes as columns -> the (6 N, 6 N) matrix"""
    rows, cidx = np.repeat(np.arange(N), N), np.tile(np.arange(N), N)
    return F.inverse_columns(np.arange(N), rows, cidx).reshape(N, N, 6, 6).transpose(0, 2, 1, 3).reshape(6 * N, 6 * N)


@functools.lru_cache(maxsize=None)
def gather_case():
    """the 40-keyframe system of tests/test_sparse_selinv_host.py (keyframes 3 and 39 outside it) and the reference of a few of its blocks, (5, 30) among them"""
    ins, hi, lo, diag, blocks, A = block_system(GATHER_N, (3, GATHER_N - 1), 2)
    pairs = [(10, 10), (5, 30), (30, 5), (10, 9), (37, 2), (0, 38), (38, 0), (20, 20)]
    return ins, hi, lo, diag, blocks, A, dref.Reference(A, pairs)


GATHER_REQUEST = [(10, 10), (5, 30), (30, 5), (10, 9), (37, 2), (0, 38), (38, 0), (20, 20), (3, 10), (10, 3), (39, 39), (5, 39)]


def check_block_gather(tag, F, ins, R):
    """what the host test and the GPU test both ask of the 40-keyframe system; F has a factor"""
    out = sc.cross_blocks(F, GATHER_REQUEST)
    live = [k for k, (a, b) in enumerate(GATHER_REQUEST) if ins[a] and ins[b]]
    assert [GATHER_REQUEST[k] for k in live] == [tuple(p) for p in R.pairs]
    e = R.error(out[live])
    info = F.columns_info()
    print("SPARSE panel gather %-22s %d blocks  launches %d  products %d  chunks %d  e %.3e  e_np %.3e  bound %g e_np" % (tag, len(out), info["launches"], info["tile_products"], info["chunks"], e, R.e_np, MARGIN))
    dref.check_exact_structure(GATHER_REQUEST, out)      # (a, b) and (b, a): exact transposes; a diagonal block: exactly symmetric
    for k, (a, b) in enumerate(GATHER_REQUEST):
        if not (ins[a] and ins[b]):
            assert np.all(out[k] == 0.0), (a, b)      # a keyframe outside the system, as row or as column: a zero block
    assert e <= R.bound
    return out


@pytest.mark.parametrize("ordering", [0, 1])
def test_blocks_of_any_pair_on_the_40_keyframe_system(shim, ordering):
    ins, hi, lo, diag, blocks, A, R = gather_case()
    H = HostColumns(shim, GATHER_N, ins, hi, lo, ordering)
    assert H.h
    H.inverse_columns([10], [5], [0])
    assert H.rc == sc.ERR_STATE      # no factor yet
    assert H.factor(diag, blocks)
    check_block_gather("host, ordering %d" % ordering, H, ins, R)
    # the column side: the side with fewer distinct keyframes, the second elements on a tie
    X = whole_inverse_blocks(H, GATHER_N)
    asked = []

    class Recorder:
        def inverse_columns(self, col_nodes, row_nodes, col_index):
            asked.append((list(col_nodes), len(row_nodes)))
            return H.inverse_columns(col_nodes, row_nodes, col_index)

    for pairs, cols, n_blocks in (([(1, 7), (2, 7), (4, 7)], [7], 3), ([(7, 1), (7, 2), (7, 4)], [7], 3), ([(1, 7), (2, 8)], [7, 8], 2), ([(1, 7), (7, 1), (1, 1), (1, 7)], [1, 7], 2)):
        got = sc.cross_blocks(Recorder(), pairs)
        assert asked[-1] == (cols, n_blocks), (pairs, asked[-1])      # every block is gathered once
        assert all(np.allclose(got[k], X[6 * a:6 * a + 6, 6 * b:6 * b + 6], rtol=0, atol=1e-15) for k, (a, b) in enumerate(pairs))
    # refusals leave `out` alone
    for cn, rn, ci in (([GATHER_N], [5], [0]), ([-1], [5], [0]), ([10], [GATHER_N], [0]), ([10, 10], [5], [0]), ([10], [5], [1]), ([10], [5], [-1])):
        out = H.inverse_columns(cn, rn, ci, fill=7.0)
        assert H.rc == sc.ERR_INVALID_ARG and np.all(out == 7.0), (cn, rn, ci)
    H.set_workspace_limit(64 * 64 * H.nt() * 8 - 1)      # below one panel
    out = H.inverse_columns([10], [5], [0], fill=7.0)
    assert H.rc == sc.ERR_INVALID_ARG and np.all(out == 7.0)
    H.close()


@pytest.mark.parametrize("ordering", [0, 1])
def test_a_column_gets_the_same_bits_alone_in_a_batch_and_in_chunks(shim, ordering):
    ins, hi, lo, diag, blocks, A, R = gather_case()
    N = GATHER_N
    H = HostColumns(shim, N, ins, hi, lo, ordering)
    assert H.h and H.factor(diag, blocks)
    rows = np.arange(N)
    alone = H.inverse_columns([10], rows, np.zeros(N, np.int32))
    one = H.columns_info()
    batch = whole_inverse_blocks(H, N)
    whole = H.columns_info()
    H.set_workspace_limit(64 * 64 * H.nt() * 8)      # one panel: ten keyframes per chunk
    chunked = whole_inverse_blocks(H, N)
    parts = H.columns_info()
    B = np.zeros((6, 6 * N)); B[np.arange(6), 60 + np.arange(6)] = 1.0
    sweeps = H.solve(B)      # ScHost's two sweeps of node 10's unit columns: rows = right-hand sides
    H.close()
    col10 = alone.reshape(6 * N, 6)      # the rows of every keyframe, the six columns of keyframe 10
    d = np.sqrt(np.diag(np.linalg.inv(A)))
    apart = float((np.abs(col10 - sweeps.T) / np.outer(d, d[60:66])).max())
    print("SPARSE panel bits ordering %d: alone %s  all 40 columns %s  in chunks %s  node 10 against the two sweeps: %.3e (bound %g e_np = %.3e)" % (ordering, one, whole, parts, apart, 2 * MARGIN, 2 * R.bound))
    assert one["chunks"] == 1 and whole["chunks"] == 1 and parts["chunks"] >= 3 and parts["bytes"] <= 64 * 64 * 4 * 8 < whole["bytes"]
    assert same_bits(col10, batch[:, 60:66]) and same_bits(batch, chunked)
    assert parts["tile_products"] >= whole["tile_products"] and parts["launches"] > whole["launches"]
    assert apart <= 2.0 * R.bound


@pytest.mark.parametrize("name", ["band_odd", "arrow"])
def test_a_matrix_as_a_block_system_gives_the_whole_inverse(shim, name):
    """the form the GPU test feeds the kernels with: the host on the very same plan"""
    A, S_ref, S_np = reference(name)
    n = len(A)
    N, hi, lo, diag, blocks = as_block_system(A)
    for ordering in (0, 1):
        H = HostColumns(shim, N, np.ones(N, np.uint8), hi, lo, ordering)
        assert H.h and H.factor(diag, blocks)
        X = whole_inverse_blocks(H, N)
        info = H.columns_info()
        H.close()
        e, e_np = scaled(X[:n, :n], S_ref), scaled(S_np, S_ref)
        print("SPARSE panel host blocks %-12s ordering %d  n %3d  launches %d  products %d  e %.3e  e_np %.3e  e / e_np %.2f" % (name, ordering, n, info["launches"], info["tile_products"], e, e_np, e / e_np))
        pad = np.arange(n, 6 * N)
        assert np.all(X[pad][:, pad] == np.eye(len(pad))) and np.all(X[pad, :n] == 0.0) and np.all(X[:n, pad] == 0.0)
        assert e <= MARGIN * e_np


# ---- cross_covariance's and the gate's host halves on a Gauss-Newton system
@functools.lru_cache(maxsize=None)
def _full_24():
    g, free, rel, sw, diag, off, c, h = gauss_newton_case()
    return full_matrix_of(g.n_poses, free, rel, sw, diag, off, c, h)


def R_matrix():
    return _full_24()[0]


def R_rows():
    return _full_24()[1]


@functools.lru_cache(maxsize=None)
def gauss_newton_cross():
    """the 24-keyframe chain with constant keyframes 4 and 23: pairs that share no edge, both ways round, diagonal blocks, pairs with a constant keyframe; the
    refined inverse of the FULL matrix (poses and switches) over the live ones"""
    g, free, rel, sw, diag, off, c, h = gauss_newton_case()
    N = g.n_poses
    pairs = [(0, 22), (22, 0), (1, 17), (9, 9), (2, 20), (20, 2), (10, 11), (11, 10), (4, 9), (9, 23), (4, 4), (0, 0), (22, 22), (17, 17), (1, 1)]
    live = [(a, b) for a, b in pairs if free[a] and free[b]]
    H, rows_of = full_matrix_of(N, free, rel, sw, diag, off, c, h)
    return pairs, live, pref.FullReference(H, live, rows_of)


@pytest.mark.parametrize("ordering", [0, 1])
def test_cross_blocks_and_the_gate_on_the_gauss_newton_case(shim, ordering):
    g, free, rel, sw, diag, off, c, h = gauss_newton_case()
    N = g.n_poses
    pairs, live, R = gauss_newton_cross()
    hi, lo, sd, sb = host_reduce(load_companion_shim(), N, free, diag, off, c, h, rel, sw)
    H = HostColumns(shim, N, free, hi, lo, ordering)
    assert H.h and H.factor(sd, sb)
    out = sc.cross_blocks(H, pairs)
    info = H.columns_info()
    e = R.error([out[k] for k, p in enumerate(pairs) if p in live])
    routed = sc._Routed(H)      # cross_covariance's rule: this few column keyframes go to the solve of their unit columns
    by_solve = sc.cross_blocks(routed, pairs)
    e_solve = R.error([by_solve[k] for k, p in enumerate(pairs) if p in live])
    print("SPARSE panel cross, host, ordering %d: the same pairs through %s (fewer than %d column keyframes): e %.3e" % (ordering, routed.route, sc.SOLVE_BELOW_COLUMNS, e_solve))
    assert routed.route == "solve" and e_solve <= R.bound
    pref.check_exact_structure(pairs, by_solve)
    assert all(np.all(by_solve[k] == 0.0) for k, (a, b) in enumerate(pairs) if not (free[a] and free[b]))
    print("SPARSE panel cross, host, 24 keyframes, constant %s, ordering %d: %d pairs  launches %d  products %d  e %.3e  e_np %.3e  e / e_np %.2f  bound %g e_np"
          % (CONSTANT_24, ordering, len(pairs), info["launches"], info["tile_products"], e, R.e_np, e / R.e_np, MARGIN))
    assert out.shape == (len(pairs), 6, 6)
    pref.check_exact_structure(pairs, out)
    assert all(np.all(out[k] == 0.0) for k, (a, b) in enumerate(pairs) if not (free[a] and free[b])) and len(live) < len(pairs)
    assert e <= R.bound
    # the gate: candidates (0, 22), (1, 17), (2, 20) with random near-identity Jacobians and random weighted residuals
    cand = [(0, 22), (1, 17), (2, 20)]
    rng = np.random.default_rng(7)
    J1, J2, r = np.eye(6) + 0.3 * rng.standard_normal((3, 6, 6)), -np.eye(6) + 0.3 * rng.standard_normal((3, 6, 6)), rng.standard_normal((3, 6))
    own = sc.cross_blocks(H, [(a, a) for a, _ in cand] + [(b, b) for _, b in cand])
    G = sc.gate_from_blocks(r, J1, J2, own[:3], own[3:], sc.cross_blocks(H, cand))
    H.close()

    def innovation(block, dtype):
        S = np.zeros((3, 6, 6), dtype)
        for k, (a, b) in enumerate(cand):
            A1, A2 = J1[k].astype(dtype), J2[k].astype(dtype)
            X = A1 @ block(a, b).astype(dtype) @ A2.T
            S[k] = A1 @ block(a, a).astype(dtype) @ A1.T + X + X.T + A2 @ block(b, b).astype(dtype) @ A2.T + np.eye(6, dtype=dtype)
        return S

    Rg = pref.FullReference(R_matrix(), [(a, a) for a, _ in cand] + [(b, b) for _, b in cand] + cand, R_rows())
    S_ref = innovation(lambda a, b: Rg.S[np.ix_(Rg.at[a], Rg.at[b])], np.longdouble)
    Lmat = np.linalg.cholesky(R_matrix())
    Linv = scipy.linalg.solve_triangular(Lmat, np.eye(len(Lmat)), lower=True)
    rows = R_rows()
    S_np = innovation(lambda a, b: Linv[:, list(rows(a))].T @ Linv[:, list(rows(b))], np.float64)
    err = lambda S: max(float((np.abs(S[k].astype(np.longdouble) - S_ref[k]) / np.sqrt(np.outer(np.diag(S_ref[k]), np.diag(S_ref[k])))).max()) for k in range(3))
    e_S, e_S_np = err(G.innovation_cov), err(S_np)
    again = np.array([r[k] @ np.linalg.solve(G.innovation_cov[k], r[k]) for k in range(3)])
    rel_d2 = float(np.abs(G.mahalanobis2 - again).max() / np.abs(again).max())
    print("SPARSE panel gate, host, ordering %d: d^2 %s  against r^T solve(S, r) %.3e relative  S: e %.3e  e_np %.3e  bound %g e_np" % (ordering, np.array2string(G.mahalanobis2, precision=4), rel_d2, e_S, e_S_np, MARGIN))
    assert G.residual.shape == (3, 6) and G.cross.shape == (3, 6, 6) and G.innovation_cov.shape == (3, 6, 6) and G.mahalanobis2.shape == (3,)
    assert all(np.array_equal(S, S.T) for S in G.innovation_cov) and all(np.all(np.linalg.eigvalsh(S) > 1.0) for S in G.innovation_cov)      # J Sigma J^T is positive definite, plus I
    assert rel_d2 <= 1e-12
    # S is a sum of congruences of the covariance blocks plus the identity: formed alike from plain numpy's blocks it sits at e_np of ITS blocks; the project's margin on that
    assert e_S <= MARGIN * e_S_np


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# the same code in a sanitized stand-alone program; the library's new symbols
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_stand_alone_program_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "sparse_panel_host_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DSPH_MAIN", "-I", CSRC, "-o", exe, SRC])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-2000:] + out.stderr[-2000:]


def test_the_library_builds_and_exports_the_columns_of_the_inverse():
    """libpgo_sparse.so cross-compiles without a GPU, exports the three new symbols and its header declares them; libpgo.so is built from what it was built from"""
    lib = sc.load()
    txt = open(os.path.join(ROOT, "include", "pgo_sparse.h")).read()
    for name in ("pgo_sparse_chol_inverse_columns", "pgo_sparse_chol_columns_info", "pgo_sparse_chol_set_workspace_limit"):
        assert name in _build.SPARSE_EXPORTS and hasattr(lib, name) and (" %s(" % name) in txt, name
    assert "PGO_SPARSE_WORKSPACE_BYTES ((int64_t)1 << 30)" in txt and sc.WORKSPACE_BYTES == 1 << 30
    assert _build.SPARSE_SOURCE not in _build.HIP_SOURCES and not set(_build.SPARSE_HEADERS) - {"pgo_dense_math.hpp"} & set(_build.HIP_HEADERS)
    assert all(hasattr(sc.SparseCholesky, f) for f in ("inverse_columns", "columns_info", "set_workspace_limit"))
    assert callable(sc.cross_covariance) and callable(sc.loop_candidate_gate) and callable(sc.cross_blocks) and callable(sc.gate_from_blocks)
