"""CPU: the arithmetic of pgo_covariance (csrc/pgo_dense_math.hpp: the request plan with switch rows, the right-hand sides, the Gram products of 6- and 1-row blocks, the
matrix-free handle's matrix from its normal blocks) instantiated serially on the host by tests/native/param_cov_host.cpp.  Host logic coverage: the product computes
covariances on the GPU only (tests/test_gpu_param_covariance.py).

Bound of the blocks: 8 x e_np against the refined inverse of the FULL matrix with the switches (tests/param_cov_ref.py).  Bound of the matrix entries: derived from the
number of summands, below.  Every test prints its figures (`PARAMCOV ...`) before it asserts."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from solve_keyframe_pose_graph_amd import capi
from tests import param_cov_ref as pref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "param_cov_host.cpp")
INC = os.path.join(ROOT, "solve_keyframe_pose_graph_amd", "csrc")
dp, ip, bp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_ubyte)
I32 = lambda x: np.ascontiguousarray(x, dtype=np.int32)
F64 = lambda x: np.ascontiguousarray(x, dtype=np.float64)


@pytest.fixture(scope="module")
def shim():
    so = os.path.join(HERE, "native", "libparam_cov_host.so")
    hdr = os.path.join(INC, "pgo_dense_math.hpp")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(SRC), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", INC, "-o", so, SRC])
    lib = C.CDLL(so)
    lib.pcv_mf_matrix.restype = C.c_longlong
    return lib


def host_covariance(shim, S, nodes, c, h, pairs, skip=True, fill=0.0):
    S, nodes, c, h = F64(S), I32(nodes), F64(c), F64(h)
    pr = I32(pairs).reshape(-1, 2)
    ia, ib = I32(pr[:, 0]), I32(pr[:, 1])
    cov = np.full((len(pr), 36), fill)
    ok = shim.pcv_covariance(C.c_int(S.shape[0]), S.ctypes.data_as(dp), nodes.ctypes.data_as(ip), c.ctypes.data_as(dp), h.ctypes.data_as(dp), C.c_longlong(len(pr)),
                             ia.ctypes.data_as(ip), ib.ctypes.data_as(ip), C.c_int(1 if skip else 0), cov.ctypes.data_as(dp))
    return bool(ok), cov


def shaped(n, pairs, cov):
    dim = lambda i: 6 if i < n // 6 else 1
    out = []
    for (a, b), row in zip(pairs, cov):
        assert np.all(row[dim(a) * dim(b):] == 0.0), (a, b)      # the rest of the fixed stride
        out.append(row[:dim(a) * dim(b)].reshape(dim(a), dim(b)))
    return out


@pytest.mark.parametrize("n", [64, 66, 192])      # one tile; 66 rows padded to 128, node 10 across the tile edge; three tiles
def test_blocks_against_the_refined_inverse_of_the_full_matrix(shim, n):
    S, nodes, c, h = pref.spd_case(n)
    pairs = pref.spd_pairs(n, len(h))
    R = pref.FullReference(pref.full_matrix(S, nodes, c, h), pairs, pref.spd_rows_of(n))
    ok, cov = host_covariance(shim, S, nodes, c, h, pairs)
    assert ok
    blocks = shaped(n, pairs, cov)
    e = R.error(blocks)
    print("PARAMCOV host n %4d + %d switches  e %.3e  e_np %.3e  bound 8 e_np %.3e" % (n, len(h), e, R.e_np, R.bound))
    assert e <= R.bound
    pref.check_exact_structure(pairs, blocks)
    k = pairs.index((n // 6 + 6, n // 6 + 6))      # a switch without a node: 1 / h alone, and no covariance with anything
    assert blocks[k][0, 0] == 1.0 / h[6] and np.all(blocks[pairs.index((3, n // 6 + 6))] == 0.0)


@pytest.mark.parametrize("n", [64, 66, 192])
def test_zero_skipping_does_not_change_a_bit(shim, n):
    S, nodes, c, h = pref.spd_case(n)
    N = n // 6
    for pairs in (pref.spd_pairs(n, len(h)), [(N + 5, N + 5)], [(N + 6, N + 6)], [(N + s, N - 1) for s in range(len(h))]):
        _, with_skip = host_covariance(shim, S, nodes, c, h, pairs, True)
        _, without = host_covariance(shim, S, nodes, c, h, pairs, False)
        assert np.array_equal(with_skip, without)


def test_the_transposed_pair_is_the_exact_transpose_for_every_combination_of_sizes(shim):
    n = 192
    S, nodes, c, h = pref.spd_case(n)
    N = n // 6
    ids = list(range(0, N, 5)) + [N + s for s in range(len(h))]
    pairs = [(a, b) for a in ids for b in ids]
    _, cov = host_covariance(shim, S, nodes, c, h, pairs)
    _, covT = host_covariance(shim, S, nodes, c, h, [(b, a) for a, b in pairs])
    shapes = set()
    for x, y, (a, b) in zip(shaped(n, pairs, cov), shaped(n, [(b, a) for a, b in pairs], covT), pairs):
        assert np.array_equal(y, x.T), (a, b)
        shapes.add(x.shape)
    assert shapes == {(6, 6), (6, 1), (1, 6), (1, 1)}


def test_pose_pose_blocks_are_the_bits_of_the_pose_only_routine(shim):
    """the rows of W do not interact: the switch rows beside them change no bit of the keyframes' blocks — requested alone with the switch columns known, and through
    tests/native/dense_cov_host.cpp, the request of pgo_pose_covariance: no switches at all.  One tile; padding and node 10 across the tile edge; three tiles."""
    so = os.path.join(HERE, "native", "libdense_cov_host.so")
    src = os.path.join(HERE, "native", "dense_cov_host.cpp")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(os.path.join(INC, "pgo_dense_math.hpp"))):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", INC, "-o", so, src])
    pose_only = C.CDLL(so)
    for n in (64, 66, 192):
        S, nodes, c, h = pref.spd_case(n)
        N = n // 6
        last, mid = N - 1, min(10, N - 1)
        pp = [(0, 0), (last, last), (mid, mid), (0, last), (1, last - 1), (last - 1, 1)]
        pairs = pp + [(N + s, N + s) for s in range(len(h))] + [(7, N + 3)]
        _, cov = host_covariance(shim, S, nodes, c, h, pairs)
        ok, alone = host_covariance(shim, S, nodes, c, h, pp)
        ia, ib = I32([a for a, _ in pp]), I32([b for _, b in pp])
        want = np.zeros((len(pp), 36))
        assert pose_only.dcv_covariance(C.c_int(n), F64(S).ctypes.data_as(dp), C.c_longlong(len(pp)), ia.ctypes.data_as(ip), ib.ctypes.data_as(ip), C.c_int(1), want.ctypes.data_as(dp)) == 1
        assert ok and np.isfinite(want).all() and np.all(want[:3, 0] > 0.0), n      # (the first three pairs: variances)
        assert np.array_equal(cov[:len(pp)], alone) and np.array_equal(cov[:len(pp)], want), n


def test_a_bad_h_and_an_indefinite_matrix_are_reported_and_nothing_is_written(shim):
    n = 66
    S, nodes, c, h = pref.spd_case(n)
    N = n // 6
    for bad in (0.0, -1.0, np.inf, np.nan):
        hb = h.copy(); hb[2] = bad
        ok, cov = host_covariance(shim, S, nodes, c, hb, [(0, 0), (N + 2, 3)], fill=7.0)
        assert not ok and np.all(cov == 7.0), bad
        ok, cov = host_covariance(shim, S, nodes, c, hb, [(0, 0), (N + 3, 3)], fill=7.0)      # nobody asked for switch 2
        assert ok and np.isfinite(cov).all(), bad
    A = np.eye(128); A[70, 70] = -1.0
    ok, cov = host_covariance(shim, A, nodes, c, h, [(3, 3)], fill=7.0)
    assert not ok and np.all(cov == 7.0)


def test_the_plan_orders_the_rows_by_their_first_column(shim):
    """24 nodes (n = 192: three tiles), 70 switches whose lower nodes spread over the matrix, every id requested: W has four tile rows; each tile row's first non-zero
    column ascends, a node's six rows stay together, a switch row sits in front of the rows of its lower node, all-zero rows come last"""
    n, N, ns = 192, 24, 70
    rng = np.random.default_rng(5)
    nodes = np.array([sorted(rng.choice(N, 2, replace=False))[::(1 if s % 2 else -1)] for s in range(ns)], dtype=np.int32)
    nodes[11] = (-1, -1); nodes[12] = (-1, 7)
    ids = I32(rng.permutation(N + ns))
    col = np.zeros(6 * N + ns + 64, np.int32); first = np.zeros_like(col); start = np.zeros(8, np.int32)
    m = shim.pcv_plan(C.c_int(n), C.c_int(N), nodes.ctypes.data_as(ip), C.c_longlong(len(ids)), ids.ctypes.data_as(ip), ids.ctypes.data_as(ip), col.ctypes.data_as(ip),
                      first.ctypes.data_as(ip), start.ctypes.data_as(ip))
    assert m == 256
    col, first, start = col[:m], first[:m], start[:m // 64]
    real = 6 * N + ns
    assert np.all(col[real:] == -1) and np.all(col[:real] != -1)
    assert np.all(np.diff(first[:real]) >= 0)
    assert list(start) == [int(first[64 * R]) // 64 for R in range(4)] and list(start) == sorted(start) and len(set(start)) > 1
    unit = np.flatnonzero(col >= 0)
    assert len(unit) == 6 * N and np.array_equal(first[unit], col[unit])
    for i in range(N):
        r = int(np.flatnonzero(col == 6 * i)[0])
        assert np.array_equal(col[r:r + 6], 6 * i + np.arange(6))
    for r in np.flatnonzero(col <= -2):
        s = -2 - int(col[r])
        lo = [x for x in nodes[s] if x >= 0]
        assert first[r] == (6 * min(lo) if lo else n)
    assert first[real - 1] == n and col[real - 1] == -2 - 11


# ---- the matrix of a matrix-free handle from its normal blocks
def mf_case(seed, N, rel, sw, constant):
    rng = np.random.default_rng(seed)
    free = np.ones(N, np.uint8); free[list(constant)] = 0
    hd = rng.standard_normal((N, 6, 6)); hd = hd + hd.transpose(0, 2, 1)
    hoff = rng.standard_normal((len(rel) + len(sw), 6, 6))
    c = rng.standard_normal((len(sw), 12))
    h = rng.uniform(0.5, 2.0, len(sw))
    return free, I32(rel).reshape(-1, 2), I32(sw).reshape(-1, 2), hd, hoff, c, h


def mf_reference(N, free, rel, sw, hd, hoff, c, h, n):
    """(A, T): the matrix assembled the way dense_cov_ref.handle_matrix does it — in np.longdouble — and per entry the sum of the absolute values of its terms with their number"""
    L = np.longdouble
    A = np.zeros((n, n), L); mag = np.zeros((n, n)); cnt = np.zeros((n, n), np.int64)
    def add(r0, c0, B):
        A[r0:r0 + 6, c0:c0 + 6] += B.astype(L); mag[r0:r0 + 6, c0:c0 + 6] += np.abs(B); cnt[r0:r0 + 6, c0:c0 + 6] += 1
    for i in range(N):
        add(6 * i, 6 * i, hd[i])
    edges = [(int(a), int(b), hoff[e]) for e, (a, b) in enumerate(rel)] + [(int(a), int(b), hoff[len(rel) + e]) for e, (a, b) in enumerate(sw)]
    for a, b, B in edges:
        add(6 * a, 6 * b, B); add(6 * b, 6 * a, B.T)
    for e, (a, b) in enumerate(sw):
        v = np.zeros(6 * N, L); v[6 * a:6 * a + 6] = c[e, :6]; v[6 * b:6 * b + 6] = c[e, 6:]
        for x in (int(a), int(b)):
            for y in (int(a), int(b)):
                blk = np.outer(v[6 * x:6 * x + 6], v[6 * y:6 * y + 6]) / L(h[e])
                A[6 * x:6 * x + 6, 6 * y:6 * y + 6] -= blk; mag[6 * x:6 * x + 6, 6 * y:6 * y + 6] += np.abs(blk).astype(np.float64); cnt[6 * x:6 * x + 6, 6 * y:6 * y + 6] += 1
    for i in range(n):
        if i >= 6 * N or not free[i // 6]:
            A[i, :] = 0; A[:, i] = 0; A[i, i] = 1; mag[i, :] = 0; mag[:, i] = 0
    return A, mag, cnt


MF_CASES = {
    # parallel edges on one pair in both orders, relative-pose and switchable mixed (two switchable loops plus an odometry edge on (2, 5))
    "parallel": (6, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (2, 5), (5, 2), (1, 0)], [(5, 2), (2, 5), (0, 5), (4, 1)], ()),
    # constant endpoints: edges into keyframes 2 and 7 vanish from the off-diagonal blocks, their switch sides stay on the free keyframe's diagonal block
    "constant": (12, [(i, i + 1) for i in range(11)] + [(0, 7), (7, 3)], [(2, 9), (9, 2), (11, 0), (7, 2), (10, 11), (11, 10)], (2, 7)),
}


@pytest.mark.parametrize("name", sorted(MF_CASES))
def test_matrix_free_matrix_from_the_normal_blocks(shim, name):
    """Bound per entry: a sum of k terms accumulated in fp64 in list order is within (k - 1) u sum|terms| of the exact sum to first order, each switch term carries two more
    roundings (product, division): (k + 1) eps sum|terms| with eps = 2 u covers both; the reference is formed in np.longdouble, so its own error does not count."""
    N, rel, sw, constant = MF_CASES[name]
    free, rel, sw, hd, hoff, c, h = mf_case(3, N, rel, sw, constant)
    n = (6 * N + 63) // 64 * 64
    A = np.zeros((n, n))
    segs = shim.pcv_mf_matrix(C.c_longlong(N), free.ctypes.data_as(bp), C.c_longlong(len(rel)), I32(rel[:, 0]).ctypes.data_as(ip), I32(rel[:, 1]).ctypes.data_as(ip),
                              C.c_longlong(len(sw)), I32(sw[:, 0]).ctypes.data_as(ip), I32(sw[:, 1]).ctypes.data_as(ip), F64(hd).ctypes.data_as(dp), F64(hoff).ctypes.data_as(dp),
                              F64(c).ctypes.data_as(dp), F64(h).ctypes.data_as(dp), C.c_int(n), A.ctypes.data_as(dp))
    want, mag, cnt = mf_reference(N, free, rel, sw, hd, hoff, c, h, n)
    pairs = {(max(a, b), min(a, b)) for a, b in np.vstack([rel, sw]) if free[a] and free[b]}
    assert segs == len(pairs)
    low = np.tril(np.ones((n, n), bool))
    for i in range(N):
        low[6 * i:6 * i + 6, 6 * i:6 * i + 6] = True      # the diagonal blocks are written whole
    assert np.all(A[~low] == 0.0)
    err = np.abs(A.astype(np.longdouble) - want)[low].astype(np.float64)
    bound = ((cnt + 1) * np.finfo(np.float64).eps * mag)[low]
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print("PARAMCOV matrix %-8s n %3d  %d off-diagonal blocks  worst error / bound %.3f  (up to %d terms per entry)" % (name, n, segs, worst, cnt.max()))
    assert np.all(err <= bound)
    for i in range(N):
        D = A[6 * i:6 * i + 6, 6 * i:6 * i + 6]
        assert np.array_equal(D, D.T)


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "param_cov_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DMAIN", "-I", INC, "-o", exe, SRC])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-2000:]


def test_public_names_of_the_parameter_covariance():
    lib = capi.load()
    assert hasattr(lib, "pgo_covariance") and hasattr(lib, "pgo_dense_spd_param_covariance")
    assert hasattr(capi.Problem, "covariance") and hasattr(capi.Problem, "dense_spd_param_covariance")
    txt = open(os.path.join(ROOT, "include", "pgo.h")).read()
    assert "int pgo_covariance(" in txt and "int pgo_dense_spd_param_covariance(" in txt and "#define PGO_ABI_VERSION 7" in txt
