"""CPU: the yaw/pitch/roll-weighted relative-pose edge (reference FourDOFError, src/CeresResidues.h:252-333, created at src/PoseGraphSLAM.cpp:1630) against the 50-digit goldens of
tests/golden/make_ypr_goldens.py: the numpy model of tests/ypr_model.py and, separately, csrc/pgo_device_math.hpp instantiated on the host by
tests/native/ypr_host.cpp (relpose_residual_ypr, its robust and cost-only forms, and the matrix-free product from the compact record).  Host logic coverage: no kernel of
the library builds this edge yet.

Bound for residuals and Jacobian blocks: 1e-12 x max(1, largest |entry| of the block), the bound of the project's parity tests.  Observed on the 60 cases (printed by the tests):
the model within 2.9e-14 (residuals) and 3.0e-15 (blocks), the host instantiation within 1.9e-14 and 2.7e-15; the matrix-free product within 2.3e-15."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from tests import ypr_model as ym

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
dp = C.POINTER(C.c_double)
BOUND = 1e-12


@pytest.fixture(scope="module")
def shim():
    so = os.path.join(HERE, "native", "libypr_host.so")
    src = os.path.join(HERE, "native", "ypr_host.cpp")
    hdr = os.path.join(ROOT, "solve_keyframe_pose_graph_amd", "csrc", "pgo_device_math.hpp")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", os.path.dirname(hdr), "-o", so, src])
    return C.CDLL(so)


@pytest.fixture(scope="module")
def goldens():
    with open(os.path.join(HERE, "golden", "ypr_goldens.json")) as f:
        d = json.load(f)
    cases = d["cases"]
    assert len(cases) >= 55
    ypr = np.array([c["ypr_deg"] for c in cases])
    assert np.abs(ypr[:, 1]).max() <= d["pitch_max_deg"] == 80                       # the generator's condition
    assert np.abs(ypr[:, 0]).max() >= 169.9 and np.abs(ypr[:, 1]).max() >= 79.9 and np.abs(ypr[:, 2]).max() >= 178.9 and np.abs(ypr).max(axis=1).min() == 0.0
    assert {tuple(c["gains"]) for c in cases} == {(4.0, 10.0, 10.0), (2.5, 7.0, 1.5)}
    return cases


def A(x):
    return np.ascontiguousarray(x, dtype=np.float64)


def P(a):
    return a.ctypes.data_as(dp)


def inputs(c, flip=False):
    qo = -A(c["q_obs"]) if flip else A(c["q_obs"])
    return [A(c["q1"]), A(c["t1"]), A(c["q2"]), A(c["t2"]), qo, A(c["t_obs"])]


def host_edge(shim, c, w=None, flip=False, cost_only=False):
    x = inputs(c, flip)
    w = c["w"] if w is None else w
    r, J1, J2 = np.zeros(6), np.zeros((6, 6)), np.zeros((6, 6))
    if cost_only:
        shim.yh_relpose_cost_only(*map(P, x), C.c_double(w), P(A(c["gains"])), P(r))
        return r
    shim.yh_relpose(*map(P, x), C.c_double(w), P(A(c["gains"])), P(r), P(J1), P(J2))
    return r, J1, J2


def worst(cases, evaluate):
    """largest error of residuals and of Jacobian blocks over the cases, each relative to max(1, largest |entry| of the golden block)"""
    er = ej = 0.0
    for c in cases:
        r, J1, J2 = evaluate(c)
        er = max(er, np.abs(r - A(c["r"])).max() / max(1.0, np.abs(c["r"]).max()))
        for J, want in ((J1, A(c["J1"])), (J2, A(c["J2"]))):
            ej = max(ej, np.abs(J - want).max() / max(1.0, np.abs(want).max()))
    return er, ej


def test_numpy_model_matches_the_goldens(goldens):
    er, ej = worst(goldens, lambda c: ym.edge(*inputs(c), c["w"], c["gains"])[:3])
    print("numpy model: residuals %.3e, Jacobian blocks %.3e (relative to max(1, largest entry))" % (er, ej))
    assert er <= BOUND and ej <= BOUND
    for c in goldens:
        assert np.abs(ym.edge(*inputs(c), c["w"], c["gains"])[3] - A(c["ypr_deg"])).max() <= 1e-9


def test_host_instantiation_matches_the_goldens(shim, goldens):
    er, ej = worst(goldens, lambda c: host_edge(shim, c))
    print("relpose_residual_ypr on the host: residuals %.3e, Jacobian blocks %.3e (relative to max(1, largest entry))" % (er, ej))
    assert er <= BOUND and ej <= BOUND


def test_the_model_reads_the_observation_from_the_matrix_as_the_record_does(goldens):
    for c in goldens:
        qo, to = ym.obs_of(c["T"])
        assert np.abs(to - A(c["t_obs"])).max() == 0.0
        assert min(np.abs(qo - A(c["q_obs"])).max(), np.abs(qo + A(c["q_obs"])).max()) <= 1e-15


def test_the_sign_of_the_observed_quaternion_does_not_matter(shim, goldens):
    for c in goldens:
        for x, y in zip(host_edge(shim, c), host_edge(shim, c, flip=True)):
            assert np.array_equal(x, y)
        for x, y in zip(ym.edge(*inputs(c), c["w"], c["gains"])[:3], ym.edge(*inputs(c, True), c["w"], c["gains"])[:3]):
            assert np.array_equal(x, y)


def test_cost_only_form_returns_the_same_residual_bits(shim, goldens):
    for c in goldens:
        assert np.array_equal(host_edge(shim, c)[0], host_edge(shim, c, cost_only=True))


@pytest.mark.parametrize("loss", [("huber", 0.1), ("cauchy", 1.0), ("huber", 1e3), None])
def test_robust_form_is_the_plain_form_at_weight_w_c(shim, goldens, loss):
    """The residual is linear in w, so Ceres' Corrector (rho'' <= 0) is the re-evaluation at weight w c, c = sqrt(rho'(s)) — c taken in numpy from the model's s"""
    enc = 0.0 if loss is None else loss[1] if loss[0] == "huber" else -loss[1]
    scaled = 0
    for c in goldens:
        r0 = ym.edge(*inputs(c), c["w"], c["gains"], want_blocks=False)[0]
        rho, cc = ym.rho_c(loss, float(r0 @ r0))
        scaled += cc < 0.99
        want = host_edge(shim, c, w=c["w"] * cc)
        r, J1, J2, out = np.zeros(6), np.zeros((6, 6)), np.zeros((6, 6)), np.zeros(2)
        shim.yh_relpose_robust(*map(P, inputs(c)), C.c_double(c["w"]), P(A(c["gains"])), C.c_double(enc), P(r), P(J1), P(J2), P(out))
        for x, y in zip((r, J1, J2), want):
            assert np.abs(x - y).max() <= BOUND * max(1.0, np.abs(y).max()), c["tag"]
        assert abs(out[0] - rho) <= BOUND * max(1.0, rho) and abs(out[1] - cc) <= BOUND
        r2, out2 = np.zeros(6), np.zeros(2)
        shim.yh_relpose_robust_cost_only(*map(P, inputs(c)), C.c_double(c["w"]), P(A(c["gains"])), C.c_double(enc), P(r2), P(out2))
        assert np.array_equal(r, r2) and np.array_equal(out, out2)
    assert (scaled >= 20) == (loss in (("huber", 0.1), ("cauchy", 1.0)))      # these residuals are in degrees: nearly every case is beyond a = 0.1


def test_matrix_free_product_is_jt_j_of_the_blocks(shim, goldens):
    """compact_apply at either side and compact_apply_both on the edge's record against J_side^T (J1 p1 + J2 p2) formed in numpy from the same shim's blocks"""
    rng = np.random.default_rng(5)
    worst_e = 0.0
    for c in goldens:
        _, J1, J2 = host_edge(shim, c)
        p1, p2 = rng.normal(size=6), rng.normal(size=6)
        u = J1 @ p1 + J2 @ p2
        want1, want2 = J1.T @ u, J2.T @ u
        y1, y2, b1, b2, rec = np.zeros(6), np.zeros(6), np.zeros(6), np.zeros(6), np.zeros(22)
        shim.yh_compact(*map(P, inputs(c)), C.c_double(c["w"]), P(A(c["gains"])), P(p1), P(p2), P(y1), P(y2), P(b1), P(b2), P(rec))
        assert rec[15] > 0.0 and rec[7] == c["gains"][0] * ym.DEG and not rec[16:].any() and rec[14] == c["w"]      # (T in b's place, the flag = kappa, no r6)
        scale = max(np.abs(want1).max(), np.abs(want2).max())
        for got, want in ((y1, want1), (y2, want2), (b1, want1), (b2, want2)):
            worst_e = max(worst_e, np.abs(got - want).max() / scale)
            assert np.abs(got - want).max() <= BOUND * scale, c["tag"]
        assert np.array_equal(y1, b1) and np.array_equal(y2, b2)
    print("matrix-free product: %.3e of the largest entry" % worst_e)


def test_an_unmarked_record_takes_the_sixdof_path(shim, goldens):
    """gains (0, 0, 0): the YPR forms of compact_apply see no flag and return the bits of the plain forms (which tests/test_device_math_host.py pins)"""
    rng = np.random.default_rng(6)
    for c in goldens:
        p1, p2 = rng.normal(size=6), rng.normal(size=6)
        y1, y2, b1, b2, rec, z1, z2 = np.zeros(6), np.zeros(6), np.zeros(6), np.zeros(6), np.zeros(22), np.zeros(6), np.zeros(6)
        shim.yh_compact(*map(P, inputs(c)), C.c_double(c["w"]), P(np.zeros(3)), P(p1), P(p2), P(y1), P(y2), P(b1), P(b2), P(rec))
        shim.yh_compact_plain(*map(P, inputs(c)), C.c_double(c["w"]), P(p1), P(p2), P(z1), P(z2))
        assert not rec[15:].any()
        assert np.array_equal(y1, z1) and np.array_equal(y2, z2) and np.array_equal(b1, z1) and np.array_equal(b2, z2)
