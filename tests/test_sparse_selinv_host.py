"""CPU: the host side of the tile-sparse selected inverse (csrc/pgo_sparse_math.hpp: sc_selinv_steps, ScSelHost, ScPlan::selinv_launches / selinv_products;
csrc/pgo_sparse_blocks.hpp: the gather of 6 x 6 blocks) through tests/native/sparse_selinv_host.cpp, and sparse_cholesky.assemble_all on top of it.  The kernels run
on the GPU only (tests/test_gpu_sparse_selinv.py, which takes its matrices, references and the host instantiation from here).

Reference: tests/dense_cov_ref.py's refined inverse (np.longdouble Newton steps) over ALL columns; error measure: its scaled entrywise e, restricted to the entries
whose tile is in the pattern of L — the selected inverse has no others.  Bound: MARGIN x e_np, the project's convention, e_np being plain fp64 numpy (Cholesky factor,
triangular inverse, Gram product) on the same matrix over the same entries.  Takahashi's recurrence is the same backward-stable factor followed by substitutions and
products in another order; a plain numpy tile-level Takahashi in fp64 sits at e / e_np = 0.39 .. 1.00 on the eleven matrices below.

Block interface: a Gauss-Newton system J^T J on the 24-keyframe chain with the hand-placed switchable loop closures of tests/pose_cov_cases.py and constant keyframes,
reduced by sc_reduce_normal_blocks, against tests/param_cov_ref.py's refined inverse of the FULL matrix (poses and switches; it never forms the Schur complement).
Every test prints its figures (`SPARSE ...`) before it asserts."""
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
from tests.pose_cov_cases import LOOPS
from tests.test_sparse_cholesky_host import CASES, full, patterned
from tests.test_sparse_companion_host import GAP, block_system, host_reduce
from tests.test_sparse_companion_host import load_shim as load_companion_shim
from tests.test_sparse_companion_host import spd_solve as host_spd_solve

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "solve_keyframe_pose_graph_amd", "csrc")
SRC = os.path.join(HERE, "native", "sparse_selinv_host.cpp")
HEADERS = ("pgo_sparse_blocks.hpp", "pgo_sparse_math.hpp", "pgo_dense_math.hpp")
NB = 64
MARGIN = dref.MARGIN
dp, ip, lp, bp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_longlong), C.POINTER(C.c_ubyte)
I32 = lambda x: np.ascontiguousarray(x, dtype=np.int32)
F64 = lambda x: np.ascontiguousarray(x, dtype=np.float64)
SELECTED_INFO = ("launches", "tile_products", "bytes", "current")


def load_shim():
    so = os.path.join(HERE, "native", "libsparse_selinv_host.so")
    deps = [SRC] + [os.path.join(CSRC, h) for h in HEADERS]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, "-o", so, SRC])
    lib = C.CDLL(so)
    lib.ssh_plan_counts.restype = C.c_longlong
    lib.ssh_plan_counts.argtypes = [C.c_int, C.c_longlong, ip, ip, ip, lp, ip]
    lib.ssh_matrix.argtypes = [C.c_int, dp, ip, dp, bp, lp, dp, dp]
    lib.ssh_create.restype = C.c_void_p
    lib.ssh_create.argtypes = [C.c_longlong, bp, C.c_longlong, ip, ip, C.c_int]
    lib.ssh_destroy.argtypes = [C.c_void_p]
    lib.ssh_factor.argtypes = [C.c_void_p, dp, dp]
    lib.ssh_selected_inverse.argtypes = [C.c_void_p]
    lib.ssh_info.argtypes = [C.c_void_p, lp, ip, lp]
    lib.ssh_selected_blocks.argtypes = [C.c_void_p, C.c_longlong, ip, ip, dp, bp]
    return lib


@pytest.fixture(scope="module")
def shim():
    return load_shim()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# the matrices, their references (computed once, shared, never written to) and the error measure
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
MATRICES = dict(CASES, gap=GAP)
NAMES = sorted(MATRICES) + ["full64", "full200", "full448"]
PERMUTED = ["arrow", "band", "full444"]


def matrix(name):
    if name.startswith("full"):
        return full(int(name[4:]))[0]
    n, tiles, _ = MATRICES[name]
    return patterned(n, tiles, n)[0]


def permuted_matrix(name):
    """(A, pos): whole 6-row nodes, a random permutation of them (tests/test_sparse_cholesky_host.py's)"""
    if name.startswith("full"):
        A = full(int(name[4:]))[0]
    else:
        n, tiles, _ = CASES[name]
        n = n // 6 * 6
        A = patterned(n, tiles, n + 1)[0]
    node_pos = np.random.default_rng(5).permutation(len(A) // 6)
    return A, (6 * node_pos[:, None] + np.arange(6)[None, :]).reshape(-1)


@functools.lru_cache(maxsize=None)
def reference(name, permuted=False):
    """(A, refined inverse, plain numpy inverse): read-only"""
    A = permuted_matrix(name)[0] if permuted else matrix(name)
    n = len(A)
    S = dref.refined_columns(A, np.arange(n))
    Linv = scipy.linalg.solve_triangular(np.linalg.cholesky(A), np.eye(n), lower=True)
    Snp = Linv.T @ Linv
    for x in (A, S, Snp):
        x.setflags(write=False)
    return A, S, Snp


def masked_error(S, S_ref, mask):
    """dense_cov_ref.scaled_error over the entries of the mask"""
    d = np.sqrt(np.diag(S_ref).astype(np.float64))
    err = (np.abs(S.astype(np.longdouble) - S_ref).astype(np.float64) / np.outer(d, d))
    return float(err[mask].max())


def host_selected(shim, A, pos=None, b=None):
    """(rc, Sigma over the pattern, mask, info, x): the shim's selected inverse of A through the matrix interface's plan"""
    A = F64(A)
    n = len(A)
    S, mask, info = np.full((n, n), 7.0), np.zeros((n, n), np.uint8), np.zeros(4, np.int64)
    p = None if pos is None else I32(pos)
    bb = None if b is None else F64(b)
    x = None if b is None else np.full(n, 7.0)
    rc = shim.ssh_matrix(n, A.ctypes.data_as(dp), None if p is None else p.ctypes.data_as(ip), S.ctypes.data_as(dp), mask.ctypes.data_as(bp), info.ctypes.data_as(lp),
                         None if bb is None else bb.ctypes.data_as(dp), None if x is None else x.ctypes.data_as(dp))
    return rc, S, mask.astype(bool), dict(zip(("launches", "tile_products", "bytes", "l_tiles"), [int(v) for v in info])), x


def tile_mask(n, tiles_of_L):
    """the entries of an n x n matrix whose tile, or its mirror image, is in the list"""
    m = np.zeros((n, n), bool)
    for i, j in tiles_of_L:
        m[i * NB:(i + 1) * NB, j * NB:(j + 1) * NB] = True
    return (m | m.T)[:n, :n]


@pytest.mark.parametrize("name", NAMES)
def test_host_selected_inverse_against_the_refined_inverse(shim, name):
    A, S_ref, S_np = reference(name)
    n = len(A)
    b = np.random.default_rng(n).standard_normal(n)
    rc, S, mask, info, x = host_selected(shim, A, b=b)
    e, e_np = masked_error(S, S_ref, mask), masked_error(S_np, S_ref, mask)
    print("SPARSE selinv host %-15s n %3d  tiles of L %2d  launches %2d  products %3d  entries in the pattern %6d of %6d  e %.3e  e_np %.3e  e / e_np %.2f  (bound %g e_np)"
          % (name, n, info["l_tiles"], info["launches"], info["tile_products"], int(mask.sum()), n * n, e, e_np, e / e_np, MARGIN))
    assert rc == 1      # factored; the padding rows came back exactly 1 on the diagonal and 0 elsewhere; every diagonal tile holds both triangles with equal bits
    if name in MATRICES:
        assert info["l_tiles"] == MATRICES[name][2]
    else:
        assert mask.all()      # a full matrix: the whole inverse
    assert np.array_equal(S, S.T) and np.all(S[~mask] == 0.0) and mask.diagonal().all()
    assert e <= MARGIN * e_np
    ok, xs, _ = host_spd_solve(load_companion_shim(), A, b)
    assert ok and np.array_equal(x, xs)      # the factor survives: the solve after the selected inverse gives the bits of the solve alone


def test_the_cases_reach_an_empty_column_fill_and_a_transposed_read(shim):
    """what the matrices are there for, read off their patterns"""
    _, _, mask, info, _ = host_selected(shim, matrix("block_diagonal"))
    assert info["launches"] == 1 and info["tile_products"] == 0 and not mask[64:, :64].any()      # s_0 and s_1 empty: the inverses of the two diagonal tiles, nothing else
    _, _, mask, info, _ = host_selected(shim, matrix("fill_only_tile"))
    assert mask[128:, 64:128].all() and np.all(matrix("fill_only_tile")[128:, 64:128] == 0.0)      # tile (2, 1) exists only as fill — and its inverse is asked for
    assert info["tile_products"] == (4 + 2) + (1 + 1)      # |s_0| = 2: column(0) reads Z(1, 2) = Z(2, 1)^T
    for name in ("band_odd", "gap", "full448"):
        info = host_selected(shim, matrix(name))[3]
        nt = (len(matrix(name)) + NB - 1) // NB
        assert info["tile_products"] > 2 * (info["l_tiles"] - nt), name      # sum m (m + 1) > 2 sum m: some |s_k| >= 2, a tile read transposed


@pytest.mark.parametrize("name", PERMUTED)
def test_host_selected_inverse_under_a_permutation_of_the_nodes(shim, name):
    A, S_ref, S_np = reference(name, True)
    _, pos = permuted_matrix(name)
    rc, S, mask, info, _ = host_selected(shim, A, pos)
    e, e_np = masked_error(S, S_ref, mask), masked_error(S_np, S_ref, mask)
    print("SPARSE selinv host %-15s permuted n %3d  tiles of L %2d  launches %2d  products %3d  entries in the pattern %6d of %6d  e %.3e  e_np %.3e  e / e_np %.2f"
          % (name, len(A), info["l_tiles"], info["launches"], info["tile_products"], int(mask.sum()), A.size, e, e_np, e / e_np))
    assert rc == 1 and np.array_equal(S, S.T) and mask.diagonal().all()
    assert e <= MARGIN * e_np


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# the plan's counts and the order of the steps
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def plan_counts(shim, A):
    nt = len(A)
    ti, tj = np.nonzero(np.tril(A, -1))
    ti, tj = I32(ti), I32(tj)
    s, counts, trace = np.zeros(nt, np.int32), np.zeros(2, np.int64), np.zeros(6 * nt + 2, np.int32)
    calls = shim.ssh_plan_counts(nt, len(ti), ti.ctypes.data_as(ip), tj.ctypes.data_as(ip), s.ctypes.data_as(ip), counts.ctypes.data_as(lp), trace.ctypes.data_as(ip))
    return s, int(counts[0]), int(counts[1]), trace[:2 * calls].reshape(-1, 2)


@pytest.mark.parametrize("seed", range(8))
def test_plan_counts_and_step_order_on_random_tile_patterns(shim, seed):
    from tests.test_sparse_cholesky_host import boolean_cholesky
    rng = np.random.default_rng(seed)
    nt = int(rng.integers(1, 41))
    A = rng.random((nt, nt)) < rng.choice([0.02, 0.08, 0.3])
    A = A | A.T | np.eye(nt, dtype=bool)
    s, launches, products, trace = plan_counts(shim, A)
    L = boolean_cholesky(A)
    brute = [int(L[k + 1:, k].sum()) for k in range(nt)]
    print("SPARSE selinv plan seed %d: nt %2d  tiles of L %3d  launches %3d  products %4d" % (seed, nt, int(L.sum()), launches, products))
    assert list(s) == brute
    assert launches == 1 + sum(3 for m in brute if m) == len(trace)      # the inverses of all diagonal tiles at once, then three steps per non-empty s_k
    assert products == sum(m * m + m for m in brute)      # column(k): |s_k|^2 tile products, diag(k): |s_k|
    want = [(3, -1)]
    for k in range(nt - 1, -1, -1):      # k descending; ginv before column before diag; an empty s_k: no step, its diagonal tile is the inverse alone
        want += [(0, k), (1, k), (2, k)] if brute[k] else []
    assert [tuple(r) for r in trace] == want


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# the block interface on the host
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
class HostSelected:
    """the shim's pgo_sparse_chol_{create, factor, selected_inverse, selected_info, selected_blocks}"""

    def __init__(self, lib, N, in_system, hi, lo, ordering):
        self.lib, self.N = lib, N
        self.ins, self.hi, self.lo = np.ascontiguousarray(in_system, dtype=np.uint8), I32(hi), I32(lo)
        self.h = lib.ssh_create(N, self.ins.ctypes.data_as(bp), len(self.hi), self.hi.ctypes.data_as(ip), self.lo.ctypes.data_as(ip), ordering)

    def factor(self, diag, blocks):
        d, b = F64(diag), F64(blocks)
        return self.lib.ssh_factor(self.h, d.ctypes.data_as(dp), b.ctypes.data_as(dp)) == 1

    def selected_inverse(self):
        return self.lib.ssh_selected_inverse(self.h)

    def info(self):
        info, order, tiles = np.zeros(4, np.int64), np.zeros(self.N, np.int32), C.c_longlong(0)
        self.lib.ssh_info(self.h, info.ctypes.data_as(lp), order.ctypes.data_as(ip), C.byref(tiles))
        return dict(zip(SELECTED_INFO, [int(v) for v in info])), order, tiles.value

    def selected_blocks(self, na, nb):
        na, nb = I32(na), I32(nb)
        out, flag = np.full((len(na), 6, 6), 7.0), np.zeros(len(na), np.uint8)
        rc = self.lib.ssh_selected_blocks(self.h, len(na), na.ctypes.data_as(ip), nb.ctypes.data_as(ip), out.ctypes.data_as(dp), flag.ctypes.data_as(bp))
        return rc, out, flag.astype(bool)

    def close(self):
        if self.h:
            self.lib.ssh_destroy(self.h)
            self.h = None


GATHER_N = 40
# node 10 (rows 60 - 65) straddles the first tile boundary; (2, 37) is a pair of the system; keyframes 3 and 39 are outside it; (5, 30) share no block
GATHER_PAIRS = [(10, 10), (0, 0), (38, 38), (10, 9), (9, 10), (10, 11), (11, 10), (37, 2), (2, 37), (20, 1), (1, 20), (3, 3), (3, 10), (10, 39), (5, 30), (30, 5)]


@functools.lru_cache(maxsize=None)
def gather_system():
    ins, hi, lo, diag, blocks, A = block_system(GATHER_N, (3, GATHER_N - 1), 2)
    live = [(a, b) for a, b in GATHER_PAIRS if ins[a] and ins[b] and {a, b} != {5, 30}]
    return ins, hi, lo, diag, blocks, A, dref.Reference(A, live)


def check_gathered(tag, ins, out, flag, R):
    """the figures and the assertions of the gather test — the GPU test runs the same on the kernels' blocks"""
    at = {p: k for k, p in enumerate(GATHER_PAIRS)}
    far = at[(5, 30)]
    for a, b in R.pairs:
        assert flag[at[(a, b)]], (a, b)      # every diagonal block and every pair of the system, the far pairs (37, 2) and (20, 1) among them, is in the pattern
    e = R.error(np.stack([out[at[(a, b)]] for a, b in R.pairs]))
    print("SPARSE selinv gather %-22s %d blocks  in the pattern %d  the far pair (5, 30): %s  e %.3e  e_np %.3e  bound %g e_np" % (tag, len(GATHER_PAIRS), int(flag.sum()), bool(flag[far]), e, R.e_np, MARGIN))
    dref.check_exact_structure(GATHER_PAIRS, out)      # (a, b) and (b, a): exact transposes; a diagonal block: exactly symmetric
    for k, (a, b) in enumerate(GATHER_PAIRS):
        if not (ins[a] and ins[b]):
            assert flag[k] and np.all(out[k] == 0.0), (a, b)      # a keyframe outside the system: a zero block, pgo_covariance's rule
        elif not flag[k]:
            assert np.all(out[k] == 0.0), (a, b)                  # reported, not guessed
    assert flag[far] == flag[at[(30, 5)]]
    assert e <= MARGIN * R.e_np
    return e


@pytest.mark.parametrize("ordering", [0, 1])
def test_the_gather_of_blocks_across_tile_boundaries(shim, ordering):
    ins, hi, lo, diag, blocks, A, R = gather_system()
    H = HostSelected(shim, GATHER_N, ins, hi, lo, ordering)
    assert H.h and H.selected_inverse() == sc.ERR_STATE      # no factor yet
    assert H.factor(diag, blocks)
    na, nb = [a for a, _ in GATHER_PAIRS], [b for _, b in GATHER_PAIRS]
    assert H.selected_blocks(na, nb)[0] == sc.ERR_STATE and H.info()[0]["current"] == 0      # no selected inverse yet
    assert H.selected_inverse() == 0 and H.info()[0]["current"] == 1
    rc, out, flag = H.selected_blocks(na, nb)
    assert rc == 0
    check_gathered("host, ordering %d" % ordering, ins, out, flag, R)
    if ordering == 0:
        assert not flag[GATHER_PAIRS.index((5, 30))]      # natural order, a band: rows 30 - 35 against columns 180 - 185 lie in tile (2, 0), which the factor does not fill
    assert H.selected_blocks([GATHER_N], [0])[0] == sc.ERR_INVALID_ARG
    assert H.factor(diag, blocks) and H.selected_blocks(na, nb)[0] == sc.ERR_STATE      # a new factor invalidates the selected inverse
    H.close()


# ---- covariance_all's quantities on a Gauss-Newton system
CONSTANT_24 = (4, 23)      # keyframe 23 is an endpoint of two of the loop closures


def gauss_newton_case(seed=3, constant=CONSTANT_24):
    """the 24-keyframe chain with the switchable loop closures LOOPS, as normal blocks of a full-rank J: per edge J1, J2 near +-identity (H_ii += J^T J, the off-diagonal
    block J1^T J2); a switchable edge has a switch column J_s and a prior row of weight 1 (c = [J1^T J_s; J2^T J_s], h = J_s^T J_s + 1); a regulariser on keyframe 0"""
    g = pref.with_loops(24, LOOPS)
    rng = np.random.default_rng(seed)
    N = g.n_poses
    rel = np.stack([g.odom_c1, g.odom_c2], axis=1).astype(np.int32); sw = np.stack([g.loop_c1, g.loop_c2], axis=1).astype(np.int32)
    diag, off = np.zeros((N, 6, 6)), np.zeros((len(rel) + len(sw), 6, 6))
    c, h = np.zeros((len(sw), 12)), np.zeros(len(sw))
    for e, (a, b) in enumerate(np.vstack([rel, sw])):
        J1, J2 = np.eye(6) + 0.3 * rng.standard_normal((6, 6)), -np.eye(6) + 0.3 * rng.standard_normal((6, 6))
        diag[a] += J1.T @ J1; diag[b] += J2.T @ J2; off[e] = J1.T @ J2
        if e >= len(rel):
            Js = 0.5 * rng.standard_normal(6)
            c[e - len(rel)] = np.concatenate([J1.T @ Js, J2.T @ Js]); h[e - len(rel)] = Js @ Js + 1.0
    for n in np.asarray(g.reg_node, dtype=np.int64):
        diag[n] += np.eye(6)
    free = np.ones(N, np.uint8); free[list(constant)] = 0
    return g, free, rel, sw, diag, off, c, h


def full_matrix_of(N, free, rel, sw, diag, off, c, h):
    """param_cov_ref.handle_full_matrix from the arrays: (H over the free keyframes' entries and ALL switches, rows_of)"""
    S = len(sw)
    H = np.zeros((6 * N + S, 6 * N + S))
    for n in range(N):
        H[6 * n:6 * n + 6, 6 * n:6 * n + 6] = diag[n]
    for e, (a, b) in enumerate(np.vstack([rel, sw])):
        H[6 * a:6 * a + 6, 6 * b:6 * b + 6] += off[e]; H[6 * b:6 * b + 6, 6 * a:6 * a + 6] += off[e].T
    for e, (a, b) in enumerate(sw):
        H[6 * a:6 * a + 6, 6 * N + e] = H[6 * N + e, 6 * a:6 * a + 6] = c[e, :6]
        H[6 * b:6 * b + 6, 6 * N + e] = H[6 * N + e, 6 * b:6 * b + 6] = c[e, 6:]
        H[6 * N + e, 6 * N + e] = h[e]
    fr = free.astype(bool)
    keep = np.concatenate([dref.node_columns(np.flatnonzero(fr)), 6 * N + np.arange(S)]).astype(np.int64)
    at = np.cumsum(fr) - 1
    nf = 6 * int(fr.sum())
    return H[np.ix_(keep, keep)], (lambda i: range(6 * at[i], 6 * at[i] + 6) if i < N else [nf + (i - N)])


def all_pairs_and_blocks(N, free, rel, sw, res):
    """covariance_all's quantities as (pairs of block ids, blocks) for param_cov_ref.FullReference — keyframe i, or N + switchable edge — and the blocks that must be zero"""
    pairs, blocks, zeros = [], [], []
    for i in range(N):
        (pairs.append((i, i)), blocks.append(res.pose[i])) if free[i] else zeros.append(res.pose[i])
    for cross, edges, first in ((res.rel_cross, rel, None), (res.sw_cross, sw, N)):
        for e, (a, b) in enumerate(edges):
            (pairs.append((int(a), int(b))), blocks.append(cross[e])) if free[a] and free[b] else zeros.append(cross[e])
    for e, (a, b) in enumerate(sw):
        pairs.append((N + e, N + e)); blocks.append(np.array([[res.switch_var[e]]]))
        for side, n in enumerate((a, b)):
            (pairs.append((N + e, int(n))), blocks.append(res.switch_pose[e, side][None, :])) if free[n] else zeros.append(res.switch_pose[e, side])
    return pairs, blocks, zeros


@functools.lru_cache(maxsize=None)
def gauss_newton_reference():
    g, free, rel, sw, diag, off, c, h = gauss_newton_case()
    H, rows_of = full_matrix_of(g.n_poses, free, rel, sw, diag, off, c, h)
    ed = sc.Edges(rel[:, 0], rel[:, 1], sw[:, 0], sw[:, 1], np.arange(len(sw), dtype=np.int32), I32(CONSTANT_24), I32(g.reg_node))
    zero = sc.assemble_all(g.n_poses, free, np.ones(g.n_poses, bool), ed, c, h, np.zeros((g.n_poses + len(rel) + len(sw), 6, 6)))
    pairs, _, _ = all_pairs_and_blocks(g.n_poses, free, rel, sw, zero)
    return ed, pref.FullReference(H, pairs, rows_of)


@pytest.mark.parametrize("ordering", [0, 1])
def test_every_quantity_of_covariance_all_through_the_host_block_interface(shim, ordering):
    g, free, rel, sw, diag, off, c, h = gauss_newton_case()
    N = g.n_poses
    ed, R = gauss_newton_reference()
    hi, lo, sd, sb = host_reduce(load_companion_shim(), N, free, diag, off, c, h, rel, sw)
    H = HostSelected(shim, N, free, hi, lo, ordering)
    assert H.h and H.factor(sd, sb) and H.selected_inverse() == 0
    na, nb = sc.all_block_requests(N, ed)
    rc, blocks, flag = H.selected_blocks(na, nb)
    info, _, l_tiles = H.info()
    H.close()
    assert rc == 0 and flag.all()      # every keyframe's own block and every edge's block is in the pattern by construction
    res = sc.assemble_all(N, free, np.ones(N, bool), ed, c, h, blocks)
    pairs, got, zeros = all_pairs_and_blocks(N, free, rel, sw, res)
    e = R.error(got)
    print("SPARSE selinv all, host, 24 keyframes, 7 loops, constant %s, ordering %d: tiles of L %d  launches %d  products %d  %d blocks  e %.3e  e_np %.3e  e / e_np %.2f  bound %g e_np"
          % (CONSTANT_24, ordering, l_tiles, info["launches"], info["tile_products"], len(pairs), e, R.e_np, e / R.e_np, MARGIN))
    assert pairs == R.pairs and all(np.all(z == 0.0) for z in zeros) and len(zeros) > 0
    assert res.pose.shape == (N, 6, 6) and res.rel_cross.shape == (len(rel), 6, 6) and res.sw_cross.shape == (len(sw), 6, 6) and res.switch_var.shape == (len(sw),) and res.switch_pose.shape == (len(sw), 2, 6)
    assert all(np.array_equal(res.pose[i], res.pose[i].T) for i in range(N)) and np.all(res.switch_var > 0.0)
    assert e <= R.bound


def test_an_unreferenced_keyframe_gets_nan_not_an_error():
    g, free, rel, sw, diag, off, c, h = gauss_newton_case()
    N = g.n_poses + 1      # one more keyframe, referenced by nothing
    ed = sc.Edges(rel[:, 0], rel[:, 1], sw[:, 0], sw[:, 1], np.arange(len(sw), dtype=np.int32))
    ins = np.ones(N, bool); ins[-1] = False
    blocks = np.zeros((N + len(rel) + len(sw), 6, 6)); blocks[:N] = np.eye(6)
    res = sc.assemble_all(N, ins, ins, ed, c, h, blocks)
    assert np.isnan(res.pose[-1]).all() and np.isfinite(res.pose[:-1]).all() and np.isfinite(res.switch_var).all()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# the same code in a sanitized stand-alone program; the library's new symbols
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_stand_alone_program_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "sparse_selinv_host_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DSSH_MAIN", "-I", CSRC, "-o", exe, SRC])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-2000:] + out.stderr[-2000:]


def test_the_library_builds_and_exports_the_selected_inverse():
    """libpgo_sparse.so cross-compiles without a GPU, exports the three new symbols and its header declares them; libpgo.so is built from what it was built from"""
    lib = sc.load()
    txt = open(os.path.join(ROOT, "include", "pgo_sparse.h")).read()
    for name in ("pgo_sparse_chol_selected_inverse", "pgo_sparse_chol_selected_info", "pgo_sparse_chol_selected_blocks"):
        assert name in _build.SPARSE_EXPORTS and hasattr(lib, name) and (" %s(" % name) in txt, name
    assert _build.SPARSE_SOURCE not in _build.HIP_SOURCES and not set(_build.SPARSE_HEADERS) - {"pgo_dense_math.hpp"} & set(_build.HIP_HEADERS)
    assert all(hasattr(sc.SparseCholesky, f) for f in ("selected_inverse", "selected_info", "selected_blocks")) and callable(sc.covariance_all)
