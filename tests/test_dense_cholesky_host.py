"""CPU: the arithmetic of the dense Cholesky solver (csrc/pgo_dense_math.hpp: the factor of a 64 x 64 diagonal block, the triangular solves with it, the order of the
block steps) instantiated serially on the host by tests/native/dense_chol_host.cpp, against numpy; and the public names of the solver.  Host logic coverage: the product
factors and solves on the GPU only (tests/test_gpu_dense_cholesky.py).

The bound.  u = 2^-53, eta(A, b, x) = |b - A x|_inf / (|A|_inf |x|_inf + |b|_inf), n the matrix order: eta <= n u, the first-order size of the rounding bound of an
n-term fp64 inner product in any order — derived, not measured.  The residual itself is formed in extended precision (np.longdouble) so that the check's own rounding
stays out of the figure."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from solve_keyframe_pose_graph_amd import capi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
dp = C.POINTER(C.c_double)
U = 2.0 ** -53


@pytest.fixture(scope="module")
def shim():
    so = os.path.join(HERE, "native", "libdense_chol_host.so")
    src = os.path.join(HERE, "native", "dense_chol_host.cpp")
    hdr = os.path.join(ROOT, "solve_keyframe_pose_graph_amd", "csrc", "pgo_dense_math.hpp")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", os.path.dirname(hdr), "-o", so, src])
    return C.CDLL(so)


def P(a):
    return a.ctypes.data_as(dp)


def spd(n):
    """as tests/test_gpu_coarse.py::test_dense_inverse_against_numpy builds them: a stiff low-rank part plus a small damping on the diagonal"""
    rng = np.random.default_rng(n)
    B = rng.standard_normal((n, max(8, n // 2)))
    A = B @ B.T + np.diag(rng.uniform(1e-3, 1.0, n))
    return 0.5 * (A + A.T), rng.standard_normal(n)


def eta(A, b, x):
    r = b.astype(np.longdouble) - A.astype(np.longdouble) @ x.astype(np.longdouble)
    return float(np.abs(r).max() / (np.abs(A).sum(axis=1).max() * np.abs(x).max() + np.abs(b).max()))


def host_solve(shim, A, b):
    A = np.ascontiguousarray(A); b = np.ascontiguousarray(b)
    x = np.full(len(b), 7.0)
    ok = shim.dch_solve(C.c_int(len(b)), P(A), P(b), P(x))
    return bool(ok), x


@pytest.mark.parametrize("n", [64, 96, 200, 448])
def test_blocked_factor_and_solve_against_numpy(shim, n):
    A, b = spd(n)
    ok, x = host_solve(shim, A, b)
    assert ok
    e, e_ref = eta(A, b, x), eta(A, b, np.linalg.solve(A, b))
    print("DENSE host n %4d  eta %.3e = %.2f u  (numpy.linalg.solve: %.2f u; bound n u = %.3e)" % (n, e, e / U, e_ref / U, n * U))
    assert e <= n * U


def test_block_routines_against_numpy(shim):
    """one 64 x 64 diagonal block: its factor is numpy's Cholesky factor to rounding, the two triangular solves give the solution of the block system"""
    A, b = spd(64)
    l, y, x = np.zeros((64, 64)), np.zeros(64), np.zeros(64)
    assert shim.dch_block(P(np.ascontiguousarray(A)), P(b), P(l), P(y), P(x)) == 1
    ref = np.linalg.cholesky(A)
    assert np.abs(l @ l.T - A).max() <= 64 * U * np.abs(A).max()
    assert np.abs(l - ref).max() <= 1e-10 * np.abs(ref).max()
    assert eta(l, b, y) <= 64 * U and eta(A, b, x) <= 64 * U


def test_an_indefinite_matrix_and_a_nan_are_reported_not_factored(shim):
    A = np.eye(128); A[70, 70] = -1.0
    ok, x = host_solve(shim, A, np.ones(128))
    assert not ok and np.all(x == 7.0)
    A = np.eye(128); A[100, 3] = A[3, 100] = np.nan
    ok, x = host_solve(shim, A, np.ones(128))
    assert not ok and np.all(x == 7.0)
    A = np.eye(64); A[63, 63] = 0.0      # a zero pivot is not > 0 either
    ok, _ = host_solve(shim, A, np.ones(64))
    assert not ok


def test_public_names_of_the_dense_solver():
    """fails without the solver: the enum values, the limit, and the exported diagnostic"""
    assert capi.LINEAR_DENSE_CHOLESKY == 2 and capi.PRECOND_DIRECT == 3 and capi.DENSE_MAX_KEYFRAMES == 1024
    assert capi.PRECOND_DIRECT & capi.PRECOND_RETRIED == 0
    lib = capi.load()
    assert hasattr(lib, "pgo_dense_spd_solve")
    txt = open(os.path.join(ROOT, "include", "pgo.h")).read()
    assert "PGO_LINEAR_DENSE_CHOLESKY = 2" in txt and "PGO_PRECOND_DIRECT = 3" in txt and "#define PGO_DENSE_MAX_KEYFRAMES 1024" in txt
