"""CPU: the arithmetic of the covariance blocks (csrc/pgo_dense_math.hpp: the forward substitution with many right-hand sides in its block steps, the zero skipping, the
Gram product's fixed reduction tree) instantiated serially on the host by tests/native/dense_cov_host.cpp, against the refined reference of tests/dense_cov_ref.py; the
teeth of the GPU test's references; and the public names.  Host logic coverage: the product computes covariances on the GPU only (tests/test_gpu_dense_covariance.py).

Bound: 8 x e_np, e_np the error of plain fp64 numpy (Cholesky, triangular inverse, Gram) against the same reference — a margin on a figure measured on the reference,
never on the code under test.  Every test prints e, e_np and the bound before it asserts."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from solve_keyframe_pose_graph_amd import capi
from tests import dense_cov_ref as ref
from tests import precond_cases as pc
from tests import util

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "dense_cov_host.cpp")
INC = os.path.join(ROOT, "solve_keyframe_pose_graph_amd", "csrc")
dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)


@pytest.fixture(scope="module")
def shim():
    so = os.path.join(HERE, "native", "libdense_cov_host.so")
    hdr = os.path.join(INC, "pgo_dense_math.hpp")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(SRC), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", INC, "-o", so, SRC])
    return C.CDLL(so)


def host_covariance(shim, A, pairs, skip=True, fill=0.0):
    A = np.ascontiguousarray(A)
    pr = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
    ia, ib = np.ascontiguousarray(pr[:, 0]), np.ascontiguousarray(pr[:, 1])
    cov = np.full((len(pr), 6, 6), fill)
    ok = shim.dcv_covariance(C.c_int(A.shape[0]), A.ctypes.data_as(dp), C.c_longlong(len(pr)), ia.ctypes.data_as(ip), ib.ctypes.data_as(ip), C.c_int(1 if skip else 0), cov.ctypes.data_as(dp))
    return bool(ok), cov


@pytest.mark.parametrize("n", [64, 66, 192])      # one tile; 66 rows padded to 128, node 10 across the tile edge; three tiles
def test_blocks_against_the_refined_reference(shim, n):
    A = ref.spd(n)
    pairs = ref.spd_pairs(n)
    R = ref.Reference(A, pairs)
    ok, cov = host_covariance(shim, A, pairs)
    assert ok
    e = R.error(cov)
    print("DENSECOV host n %4d  e %.3e  e_np %.3e  bound 8 e_np %.3e" % (n, e, R.e_np, R.bound))
    assert e <= R.bound
    ref.check_exact_structure(pairs, cov)


@pytest.mark.parametrize("n", [64, 66, 192])
def test_zero_skipping_does_not_change_a_bit(shim, n):
    A = ref.spd(n)
    last = n // 6 - 1
    for pairs in (ref.spd_pairs(n), [(last, last)], [(a, a) for a in range(last + 1)]):
        _, with_skip = host_covariance(shim, A, pairs, True)
        _, without = host_covariance(shim, A, pairs, False)
        assert np.array_equal(with_skip, without)


def test_the_transposed_pair_is_the_exact_transpose(shim):
    A = ref.spd(192)
    pairs = [(a, b) for a in range(0, 32, 5) for b in range(0, 32, 3)]
    _, cov = host_covariance(shim, A, pairs)
    _, covT = host_covariance(shim, A, [(b, a) for a, b in pairs])
    for k in range(len(pairs)):
        assert np.array_equal(covT[k], cov[k].T)
        if pairs[k][0] == pairs[k][1]:
            assert np.array_equal(cov[k], cov[k].T)


def test_an_indefinite_matrix_is_reported_and_nothing_is_written(shim):
    A = np.eye(128); A[70, 70] = -1.0
    ok, cov = host_covariance(shim, A, [(3, 3)], fill=7.0)
    assert not ok and np.all(cov == 7.0)


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "dense_cov_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DDCV_MAIN", "-I", INC, "-o", exe, SRC])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-2000:]


# ---- teeth: the wrong references a covariance routine could be computing differ from the right one by far more than the GPU test's tolerance
def schur(H, N):
    return H[:6 * N, :6 * N] - H[:6 * N, 6 * N:] @ np.linalg.solve(H[6 * N:, 6 * N:], H[6 * N:, :6 * N]) if H.shape[0] > 6 * N else H


def lm_damping(H, radius):
    scale = 1.0 / (1.0 + np.sqrt(np.diag(H)))
    return np.clip(scale ** 2 * np.diag(H), 1e-6, 1e32) / (radius * scale ** 2), scale


def gpu_tolerance(A):
    N = A.shape[0] // 6
    return ref.Reference(A, [(a, a) for a in range(N)]).bound


def test_teeth_damping_and_scaling_on_the_22_keyframe_graph():
    g = util.small_graph(22, 3, f=3, seed=11)
    q, t, s = pc.state(g)
    H = util.oracle_problem(g, True).dense_normal_matrix(q, t, s)
    N = g.n_poses
    A = schur(H, N)
    S_ref = np.linalg.inv(A)
    tol = gpu_tolerance(A)
    lam, scale = lm_damping(H, 1e4)
    damped = np.linalg.inv(schur(H + np.diag(lam), N))
    scaled = np.linalg.inv(np.diag(scale[:6 * N]) @ A @ np.diag(scale[:6 * N]))
    e_damped, e_scaled = ref.scaled_error(damped, S_ref), ref.scaled_error(scaled, S_ref)
    print("DENSECOV teeth 22 keyframes: GPU tolerance %.3e; LM damping of radius 1e4 left in %.3e; Jacobi scaling left in %.3e" % (tol, e_damped, e_scaled))
    assert e_damped > 100.0 * tol and e_scaled > 100.0 * tol


def test_teeth_conditioning_on_the_switches():
    """on a 60-keyframe graph with 8 switchable loop closures: the 22-keyframe graph of the generator carries none (no loop fits below its minimum loop gap), so it has no
    switch to condition on"""
    g = util.small_graph(60, 8, f=2, seed=11)
    q, t, s = pc.state(g)
    H = util.oracle_problem(g, True).dense_normal_matrix(q, t, s)
    N = g.n_poses
    assert g.n_loops == 8 and H.shape[0] == 6 * N + 8
    A = schur(H, N)
    S_ref = np.linalg.inv(A)
    conditioned = np.linalg.inv(H[:6 * N, :6 * N])
    tol = gpu_tolerance(A)
    e_cond = ref.scaled_error(conditioned, S_ref)
    print("DENSECOV teeth 60 keyframes, 8 switches: GPU tolerance %.3e; pose block inverted without the Schur term %.3e" % (tol, e_cond))
    assert e_cond > 100.0 * tol


def test_public_names_of_the_covariance():
    lib = capi.load()
    assert hasattr(lib, "pgo_pose_covariance") and hasattr(lib, "pgo_dense_spd_covariance")
    assert hasattr(capi.Problem, "pose_covariance") and hasattr(capi.Problem, "dense_spd_covariance")
    txt = open(os.path.join(ROOT, "include", "pgo.h")).read()
    assert "int pgo_pose_covariance(" in txt and "int pgo_dense_spd_covariance(" in txt and "#define PGO_ABI_VERSION 7" in txt
