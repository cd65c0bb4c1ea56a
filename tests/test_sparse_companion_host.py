"""CPU: the host side of libpgo_sparse.so (csrc/pgo_sparse_blocks.hpp) through tests/native/sparse_companion_host.cpp — the reduction of a handle's normal blocks to the
blocks of the undamped Schur complement, the block interface (pair checks, fill of the permuted tiles, solve) run serially with ScHost, and a tile pattern with a hole
in s_0 that tests/test_sparse_cholesky_host.py's CASES do not have.  The kernels run on the GPU only (tests/test_gpu_sparse_cholesky.py).

Bound of the reduction's entries: a sum of k terms accumulated in fp64 in list order is within (k - 1) u sum|terms| of the exact sum to first order, each switch term
carries two more roundings (product, division): (k + 1) eps sum|terms| with eps = 2 u covers both — tests/test_param_cov_host.py's bound, whose np.longdouble
assembly (mf_reference) is the reference here.  Every test prints its figures (`SPARSE ...`) before it asserts."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from solve_keyframe_pose_graph_amd import _build
from tests import param_cov_ref as pref
from tests import precond_cases as pc
from tests.pose_cov_cases import LOOPS
from tests.test_dense_cholesky_host import U, eta
from tests.test_param_cov_host import mf_reference
from tests.test_sparse_cholesky_host import patterned

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "solve_keyframe_pose_graph_amd", "csrc")
SRC = os.path.join(HERE, "native", "sparse_companion_host.cpp")
HEADERS = ("pgo_sparse_blocks.hpp", "pgo_sparse_math.hpp", "pgo_dense_math.hpp")
INFO = ("nt", "a_tiles", "l_tiles", "ordering", "bytes", "factor_launches", "solve_launches", "tile_updates")
dp, ip, lp, bp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_longlong), C.POINTER(C.c_ubyte)
I32 = lambda x: np.ascontiguousarray(x, dtype=np.int32)
F64 = lambda x: np.ascontiguousarray(x, dtype=np.float64)

# the tile pattern the host file's CASES lack: s_0 = {2, 4} — two tiles with a hole between them, tile (4, 2) is fill; 5 diagonal tiles + 2 + 1 = 8 tiles of L.
# A panel scratch indexed by tile row instead of by position in s_0 would put tile 4's copy two tiles further than the scratch of max |s_k| = 2 tiles reaches.
GAP = (320, [(2, 0), (4, 0)], 8)


def load_shim():
    so = os.path.join(HERE, "native", "libsparse_companion_host.so")
    deps = [SRC] + [os.path.join(CSRC, h) for h in HEADERS]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, "-o", so, SRC])
    lib = C.CDLL(so)
    lib.sph_reduce.restype = C.c_longlong
    lib.sph_create.restype = C.c_void_p
    lib.sph_destroy.argtypes = [C.c_void_p]
    lib.sph_info.argtypes = [C.c_void_p, lp, ip]
    lib.sph_factor.argtypes = [C.c_void_p, dp, dp]
    lib.sph_solve.argtypes = [C.c_void_p, C.c_longlong, dp, dp]
    lib.sph_inverse_blocks.argtypes = [C.c_void_p, C.c_longlong, lp, lp, ip, dp, C.c_longlong, ip, ip, C.c_int, dp]
    return lib


@pytest.fixture(scope="module")
def shim():
    return load_shim()


def host_reduce(lib, N, free, diag, off, c, h, rel, sw):
    """(pair_hi, pair_lo, s_diag, s_blocks) of the shim"""
    E = len(rel) + len(sw)
    free = np.ascontiguousarray(free, dtype=np.uint8)
    hi, lo, sd, sb = np.zeros(E, np.int32), np.zeros(E, np.int32), np.zeros((N, 6, 6)), np.zeros((E, 6, 6))
    rel, sw = I32(rel).reshape(-1, 2), I32(sw).reshape(-1, 2)
    m = lib.sph_reduce(C.c_longlong(N), free.ctypes.data_as(bp), F64(diag).ctypes.data_as(dp), F64(off).ctypes.data_as(dp), F64(c).ctypes.data_as(dp), F64(h).ctypes.data_as(dp),
                       C.c_longlong(len(rel)), I32(rel[:, 0]).ctypes.data_as(ip), I32(rel[:, 1]).ctypes.data_as(ip), C.c_longlong(len(sw)), I32(sw[:, 0]).ctypes.data_as(ip),
                       I32(sw[:, 1]).ctypes.data_as(ip), hi.ctypes.data_as(ip), lo.ctypes.data_as(ip), sd.ctypes.data_as(dp), sb.ctypes.data_as(dp))
    return hi[:m], lo[:m], sd, sb[:m]


def random_blocks(seed, N, n_rel, n_sw):
    rng = np.random.default_rng(seed)
    hd = rng.standard_normal((N, 6, 6)); hd = hd + hd.transpose(0, 2, 1)
    return hd, rng.standard_normal((n_rel + n_sw, 6, 6)), rng.standard_normal((n_sw, 12)), rng.uniform(0.5, 2.0, n_sw)


REDUCE_CASES = {
    # two pairs of switchable loops on one pair of keyframes in both orders, (7, 9) also joined by the f = 2 odometry: one block each, the sum
    "loops24": (lambda: pref.with_loops(24, LOOPS), ()),
    "tl200_constant": (lambda: pc.graph("tl200"), tuple(range(20, 30))),
}


@pytest.mark.parametrize("name", sorted(REDUCE_CASES))
def test_the_reduction_against_a_longdouble_assembly(shim, name):
    make, constant = REDUCE_CASES[name]
    g = make()
    N = g.n_poses
    rel = np.stack([g.odom_c1, g.odom_c2], axis=1); sw = np.stack([g.loop_c1, g.loop_c2], axis=1)
    free = np.ones(N, np.uint8); free[list(constant)] = 0
    hd, hoff, c, h = random_blocks(7, N, len(rel), len(sw))
    hi, lo, sd, sb = host_reduce(shim, N, free, hd, hoff, c, h, rel, sw)
    n = 6 * N
    want, mag, cnt = mf_reference(N, free, rel, sw, hd, hoff, c, h, n)
    pairs = sorted({(int(max(a, b)), int(min(a, b))) for a, b in np.vstack([rel, sw]) if a != b and free[a] and free[b]})
    assert list(zip(hi.tolist(), lo.tolist())) == pairs      # every pair of keyframes once, sorted, however many edges join it
    edges_per_pair = len([1 for a, b in np.vstack([rel, sw]) if free[a] and free[b]]) / len(pairs)
    eps = np.finfo(np.float64).eps
    worst = 0.0
    for k, (a, b) in enumerate(pairs):
        blk = np.s_[6 * a:6 * a + 6, 6 * b:6 * b + 6]
        err = np.abs(sb[k].astype(np.longdouble) - want[blk]).astype(np.float64)
        bound = (cnt[blk] + 1) * eps * mag[blk]
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert np.all(err <= bound), (a, b)
    for i in range(N):
        blk = np.s_[6 * i:6 * i + 6, 6 * i:6 * i + 6]
        if not free[i]:
            assert np.all(sd[i] == 0.0)
            continue
        err = np.abs(sd[i].astype(np.longdouble) - want[blk]).astype(np.float64)
        bound = (cnt[blk] + 1) * eps * mag[blk]
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert np.all(err <= bound), i
        assert np.array_equal(sd[i], sd[i].T)
    print("SPARSE reduce %-15s %d keyframes  %d pairs (%.2f edges per pair, up to %d terms per entry)  worst error / bound %.3f" % (name, N, len(pairs), edges_per_pair, cnt.max(), worst))
    assert name != "loops24" or edges_per_pair > 1.0      # there are duplicates to sum


def test_duplicate_edges_give_one_pair_with_the_sum(shim):
    """three edges on keyframes (1, 3): relative-pose (1, 3), relative-pose (3, 1), switchable (3, 1); one block, rows of keyframe 3"""
    N = 4
    rel, sw = [(0, 1), (1, 3), (3, 1), (1, 2)], [(3, 1)]
    hd, hoff, c, h = random_blocks(3, N, len(rel), len(sw))
    hi, lo, sd, sb = host_reduce(shim, N, np.ones(N, np.uint8), hd, hoff, c, h, rel, sw)
    assert list(zip(hi.tolist(), lo.tolist())) == [(1, 0), (2, 1), (3, 1)]
    want = (hoff[1].T + hoff[2]) + (hoff[4] - np.outer(c[0, :6], c[0, 6:]) / h[0])      # in edge order: edge 1 transposed (its c1 is the lower keyframe), edge 2, the switchable one
    assert np.array_equal(sb[2], want)
    assert np.array_equal(sd[3], (hd[3] - np.outer(c[0, :6], c[0, :6]) / h[0]))


def spd_solve(shim, A, b, pos=None):
    A, b = F64(A), F64(b)
    x, info = np.full(len(b), 7.0), np.zeros(8, np.int64)
    p = None if pos is None else I32(pos)
    ok = shim.sph_spd_solve(C.c_int(len(b)), A.ctypes.data_as(dp), b.ctypes.data_as(dp), None if p is None else p.ctypes.data_as(ip), x.ctypes.data_as(dp), info.ctypes.data_as(lp))
    return bool(ok), x, dict(zip(INFO, [int(v) for v in info]))


def dense_solve(shim, A, b):
    A, b = F64(A), F64(b)
    x = np.full(len(b), 7.0)
    assert shim.sph_dense_solve(C.c_int(len(b)), A.ctypes.data_as(dp), b.ctypes.data_as(dp), x.ctypes.data_as(dp)) == 1
    return x


def test_a_hole_in_the_first_column_equals_the_dense_host_solve_as_numbers(shim):
    n, tiles, l_tiles = GAP
    A, b = patterned(n, tiles, n)
    ok, x, info = spd_solve(shim, A, b)
    assert ok and info["nt"] == 5 and info["a_tiles"] == 7 and info["l_tiles"] == l_tiles      # fill at (4, 2)
    assert info["factor_launches"] == 1 + 3 + 1 + 3 + 1      # step 0: panel, update, diagonal tile 1 alone; step 1: empty, diagonal tile 2; step 2: panel, update, tile 3; step 3: empty, tile 4
    e = eta(A, b, x)
    print("SPARSE host gap n %d  tiles of L %d  eta %.3e = %.2f u (bound n u = %.3e)" % (n, info["l_tiles"], e, e / U, n * U))
    assert np.array_equal(x, dense_solve(shim, A, b))
    assert e <= n * U


class HostBlocks:
    """the shim's block interface: pgo_sparse_chol_* on the host"""

    def __init__(self, lib, N, in_system, hi, lo, ordering):
        self.lib, self.N = lib, N
        self.ins, self.hi, self.lo = np.ascontiguousarray(in_system, dtype=np.uint8), I32(hi), I32(lo)
        self.h = lib.sph_create(C.c_longlong(N), self.ins.ctypes.data_as(bp), C.c_longlong(len(self.hi)), self.hi.ctypes.data_as(ip), self.lo.ctypes.data_as(ip), C.c_int(ordering))

    def info(self):
        info, order = np.zeros(8, np.int64), np.zeros(self.N, np.int32)
        self.lib.sph_info(self.h, info.ctypes.data_as(lp), order.ctypes.data_as(ip))
        return dict(zip(INFO, [int(v) for v in info])), order

    def factor(self, diag, blocks):
        d, b = F64(diag), F64(blocks)
        return self.lib.sph_factor(self.h, d.ctypes.data_as(dp), b.ctypes.data_as(dp)) == 1

    def solve(self, B):
        B = F64(B).reshape(-1, 6 * self.N)
        X = np.full_like(B, 7.0)
        self.lib.sph_solve(self.h, C.c_longlong(len(B)), B.ctypes.data_as(dp), X.ctypes.data_as(dp))
        return X

    def inverse_blocks(self, groups, pairs, skip=True):
        group_ptr, row_ptr, col, val = [0], [0], [], []
        for g in groups:
            for cols, vals in g:
                col.extend(cols); val.extend(vals); row_ptr.append(len(col))
            group_ptr.append(len(row_ptr) - 1)
        gp, rp, cc, vv = np.asarray(group_ptr, np.int64), np.asarray(row_ptr, np.int64), I32(col), F64(val)
        pr = I32(pairs).reshape(-1, 2)
        ga, gb = I32(pr[:, 0]), I32(pr[:, 1])
        out = np.zeros((len(pr), 36))
        rc = self.lib.sph_inverse_blocks(self.h, C.c_longlong(len(groups)), gp.ctypes.data_as(lp), rp.ctypes.data_as(lp), cc.ctypes.data_as(ip), vv.ctypes.data_as(dp), C.c_longlong(len(pr)),
                                         ga.ctypes.data_as(ip), gb.ctypes.data_as(ip), C.c_int(1 if skip else 0), out.ctypes.data_as(dp))
        assert rc == 0
        dim = lambda g: len(groups[g])
        return [out[k, :dim(a) * dim(b)].reshape(dim(a), dim(b)).copy() for k, (a, b) in enumerate(pr)]

    def close(self):
        if self.h:
            self.lib.sph_destroy(self.h)
            self.h = None


def block_system(N, outside, seed):
    """a chain with f = 2 odometry pairs and two far pairs, given in mixed (higher, lower) order: diagonally dominant 6 x 6 blocks; (in_system, hi, lo, diag, blocks, dense matrix)"""
    rng = np.random.default_rng(seed)
    ins = np.ones(N, np.uint8); ins[list(outside)] = 0
    pairs = [(i, j) for i in range(N) for j in (i + 1, i + 2) if j < N] + [(N - 3, 2), (N // 2, 1)]
    pairs = [(a, b) if k % 2 else (b, a) for k, (a, b) in enumerate(pairs) if ins[a] and ins[b]]
    hi, lo = I32([p[0] for p in pairs]), I32([p[1] for p in pairs])
    blocks = rng.standard_normal((len(pairs), 6, 6))
    diag = rng.standard_normal((N, 6, 6)); diag = 0.5 * (diag + diag.transpose(0, 2, 1)) + 60.0 * np.eye(6)
    A = np.zeros((6 * N, 6 * N))
    for i in range(N):
        A[6 * i:6 * i + 6, 6 * i:6 * i + 6] = diag[i] if ins[i] else np.eye(6)
    for k, (a, b) in enumerate(pairs):
        A[6 * a:6 * a + 6, 6 * b:6 * b + 6] = blocks[k]; A[6 * b:6 * b + 6, 6 * a:6 * a + 6] = blocks[k].T
    return ins, hi, lo, diag, blocks, A


@pytest.mark.parametrize("N", [10, 40])      # one tile with padding; four tiles, keyframes across the tile edges
def test_the_block_interface_in_natural_order_equals_the_matrix_interface_as_numbers(shim, N):
    ins, hi, lo, diag, blocks, A = block_system(N, (3, N - 1), N)
    H = HostBlocks(shim, N, ins, hi, lo, 0)
    assert H.h and H.factor(diag, blocks)
    B = np.random.default_rng(1).standard_normal((3, 6 * N))
    X = H.solve(B)
    info, order = H.info()
    H.close()
    outside = np.repeat(ins == 0, 6)
    assert np.array_equal(order, np.arange(N)) and info["ordering"] == 0
    for r in range(3):
        b = B[r].copy(); b[outside] = 0.0
        ok, x, minfo = spd_solve(shim, A, b)
        assert ok and np.array_equal(X[r], x) and np.all(X[r][outside] == 0.0)
    assert minfo["l_tiles"] == info["l_tiles"] and minfo["factor_launches"] == info["factor_launches"]


def test_the_block_interface_under_rcm_and_its_inverse_blocks(shim):
    N = 40
    ins, hi, lo, diag, blocks, A = block_system(N, (3, N - 1), 2)
    H = HostBlocks(shim, N, ins, hi, lo, 1)
    assert H.h and H.factor(diag, blocks)
    info, order = H.info()
    assert info["ordering"] == 1 and np.array_equal(np.sort(order), np.arange(N)) and list(order[-2:]) == [3, N - 1]
    b = np.random.default_rng(2).standard_normal(6 * N); b[np.repeat(ins == 0, 6)] = 0.0
    x = H.solve(b)[0]
    e = eta(A, b, x)
    unit = lambda i: [([6 * i + a], [1.0]) for a in range(6)]
    row = [(list(range(12, 18)) + list(range(222, 228)), list(np.linspace(-1.0, 1.0, 12)))]
    groups, pairs = [unit(38), unit(10), row], [(0, 0), (0, 1), (1, 0), (2, 2), (2, 0), (0, 2)]
    cov = H.inverse_blocks(groups, pairs)
    same = H.inverse_blocks(groups, pairs, skip=False)
    H.close()
    Ainv = np.linalg.inv(A)
    V = [np.eye(6 * N)[228:234], np.eye(6 * N)[60:66], np.zeros((1, 6 * N))]
    V[2][0, row[0][0]] = row[0][1]
    err = max(float(np.abs(c - V[a] @ Ainv @ V[b].T).max()) for c, (a, b) in zip(cov, pairs))
    print("SPARSE host blocks rcm: tiles of L %d  eta %.3e (bound n u = %.3e)  inverse blocks against numpy %.3e" % (info["l_tiles"], e, 6 * N * U, err))
    assert e <= 6 * N * U and err <= 1e-13
    assert all(np.array_equal(p, q) for p, q in zip(cov, same))      # the skipped steps would have written +0
    assert np.array_equal(cov[1], cov[2].T) and np.array_equal(cov[4], cov[5].T) and np.array_equal(cov[0], cov[0].T)


def test_bad_pair_lists_are_refused(shim):
    ins, hi, lo, _, _, _ = block_system(10, (3,), 1)
    for bad_hi, bad_lo in ((lo[0], hi[0]), (3, 5), (5, 5), (10, 0), (-1, 0)):      # listed twice (the other way round), an outside keyframe, with itself, out of range
        H = HostBlocks(shim, 10, ins, list(hi) + [bad_hi], list(lo) + [bad_lo], 0)
        assert not H.h, (bad_hi, bad_lo)


def test_the_stand_alone_program_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "sparse_companion_host_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DSPH_MAIN", "-I", CSRC, "-o", exe, SRC])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-2000:] + out.stderr[-2000:]


def test_the_library_builds_and_exports_what_its_header_declares(shim):
    """libpgo_sparse.so cross-compiles without a GPU; its host-only entry point gives the shim's bits"""
    from solve_keyframe_pose_graph_amd import sparse_cholesky as sc
    lib = sc.load()
    txt = open(os.path.join(ROOT, "include", "pgo_sparse.h")).read()
    for name in _build.SPARSE_EXPORTS:
        assert hasattr(lib, name) and (" %s(" % name) in txt, name
    assert _build.SPARSE_SOURCE not in _build.HIP_SOURCES and not set(_build.SPARSE_HEADERS[:2]) & set(_build.HIP_HEADERS)      # libpgo.so is built from what it was built from
    N, rel, sw = 4, [(0, 1), (1, 3), (3, 1), (1, 2)], [(3, 1), (0, 2)]
    hd, hoff, c, h = random_blocks(4, N, len(rel), len(sw))
    free = np.array([1, 1, 0, 1], np.uint8)
    got = sc.reduce_normal_blocks(N, free, hd, hoff, c, h, [a for a, _ in rel], [b for _, b in rel], [a for a, _ in sw], [b for _, b in sw])
    want = host_reduce(shim, N, free, hd, hoff, c, h, rel, sw)
    assert all(np.array_equal(x, y) for x, y in zip(got, want)) and len(got[0]) == 2
