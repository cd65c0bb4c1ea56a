#!/usr/bin/env python3
"""Generates tests/golden/ypr_goldens.json — the pin for the yaw/pitch/roll-weighted relative-pose edge (reference FourDOFError,
src/CeresResidues.h:252-333; R2ypr, src/utils/PoseManipUtils.cpp:143-158), which the oracle cannot evaluate.

As tests/golden/make_functor_goldens.py does for the other functors, and with its helpers:
  * residuals: what FourDOFError::operator() computes, with the reference's own R2ypr formula (cos / sin of the yaw angle), in 50 significant digits;
  * Jacobians: 50-digit central differences through the Ceres `EigenQuaternionParameterization::Plus` retraction, step 1e-20.
Nothing here knows the closed-form blocks of csrc/pgo_device_math.hpp or tests/ypr_model.py.

The cases are built from a wanted error (yaw, pitch, roll): q2 = q1 (x) q_o (x) q_err*, so that delta_q = q2* (x) q1 (x) q_o = q_err up to the rounding of q2 to doubles.
Every case has |pitch error| <= 80 degrees: a condition of this generator, asserted below (the Euler singularity at 90 degrees is the reference functor's own).

Run:  python tests/golden/make_ypr_goldens.py      (deterministic; numpy seed 20261018)
"""
import json
import os
import sys

import mpmath as mp
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_functor_goldens import fl, make_T, mat_to_quat_eigen, mpv, num_jac, plus, qconj, qmul, rand_unit_quat, rotmat  # noqa: E402

mp.mp.dps = 50
DEG = 180 / mp.pi
REFERENCE_GAINS = (4.0, 10.0, 10.0)      # CeresResidues.h:303-305
OTHER_GAINS = (2.5, 7.0, 1.5)
PITCH_MAX_DEG = 80


def r2ypr_deg(R):
    """PoseManipUtils::R2ypr, in degrees"""
    y = mp.atan2(R[1, 0], R[0, 0])
    p = mp.atan2(-R[2, 0], R[0, 0] * mp.cos(y) + R[1, 0] * mp.sin(y))
    r = mp.atan2(R[0, 2] * mp.sin(y) - R[1, 2] * mp.cos(y), -R[0, 1] * mp.sin(y) + R[1, 1] * mp.cos(y))
    return [y * DEG, p * DEG, r * DEG]


def res_ypr(q1, t1, q2, t2, qo, to, w, g):
    R1 = rotmat(q1)
    R2 = rotmat(q2)
    dt = R2.T * (mp.matrix(t1) + R1 * mp.matrix(to) - mp.matrix(t2))
    dq = qmul(qmul(qconj(q2), q1), qo)
    ypr = r2ypr_deg(rotmat(dq))
    return [w * dt[0], w * dt[1], w * dt[2], w * g[0] * ypr[0], w * g[1] * ypr[1], w * g[2] * ypr[2]]


def euler_quat(y, p, r):
    """quaternion (x, y, z, w) of Rz(y) Ry(p) Rx(r), radians"""
    cy, sy, cp, sp, cr, sr = np.cos(y / 2), np.sin(y / 2), np.cos(p / 2), np.sin(p / 2), np.cos(r / 2), np.sin(r / 2)
    return np.array([cy * cp * sr - sy * sp * cr, cy * sp * cr + sy * cp * sr, sy * cp * cr - cy * sp * sr, cy * cp * cr + sy * sp * sr])


def qmul_np(a, b):
    return np.array([float(x) for x in qmul(mpv(a), mpv(b))])


def case(rng, err_deg, w, g, flip_obs, identity_poses=False, tag=""):
    y, p, r = np.deg2rad(err_deg)
    q_err = euler_quat(y, p, r)
    if identity_poses:
        q1, qo = np.array([0, 0, 0, 1.0]), np.array([0, 0, 0, 1.0])
        t1, to = np.zeros(3), np.zeros(3)
    else:
        q1, qo = rand_unit_quat(rng), rand_unit_quat(rng)
        t1, to = rng.normal(size=3) * 5, rng.normal(size=3) * 2
    T16 = make_T(qo, to)
    # the observation the edge record holds: Eigen's quaternion of T's rotation block, or its negative (the same rotation)
    Tm = mp.matrix(3, 3)
    for c in range(3):
        for rr in range(3):
            Tm[rr, c] = mp.mpf(float(T16[c * 4 + rr]))
    q_obs = np.array([float(x) for x in mat_to_quat_eigen(Tm)])
    if flip_obs:
        q_obs = -q_obs
    q2 = qmul_np(qmul_np(q1, q_obs), q_err * np.array([-1, -1, -1, 1.0]))
    q2 = q2 / np.linalg.norm(q2)
    t2 = np.zeros(3) if identity_poses else t1 + rng.normal(size=3) * 2
    Q1, T1, Q2, T2, QO, TO, W, G = mpv(q1), mpv(t1), mpv(q2), mpv(t2), mpv(q_obs), mpv(to), mp.mpf(float(w)), mpv(g)

    def f(pp):
        a1 = pp.get("th1", [0, 0, 0]); b1 = pp.get("p1", [0, 0, 0]); a2 = pp.get("th2", [0, 0, 0]); b2 = pp.get("p2", [0, 0, 0])
        return res_ypr(plus(Q1, a1), [T1[i] + b1[i] for i in range(3)], plus(Q2, a2), [T2[i] + b2[i] for i in range(3)], QO, TO, W, G)
    res = f({})
    ypr = r2ypr_deg(rotmat(qmul(qmul(qconj(Q2), Q1), QO)))
    assert abs(ypr[1]) <= PITCH_MAX_DEG, (tag, err_deg, float(ypr[1]))
    J = num_jac(f, 6, [("th1", 3), ("p1", 3), ("th2", 3), ("p2", 3)])
    J1 = [J["th1"][i] + J["p1"][i] for i in range(6)]
    J2 = [J["th2"][i] + J["p2"][i] for i in range(6)]
    return dict(tag=tag, q1=fl(list(q1)), t1=fl(list(t1)), q2=fl(list(q2)), t2=fl(list(t2)), T=fl(list(T16)), q_obs=fl(list(q_obs)), t_obs=fl(list(to)), w=float(w),
                gains=[float(x) for x in g], ypr_deg=fl(ypr), r=fl(res), J1=fl(J1), J2=fl(J2))


def main():
    rng = np.random.default_rng(20261018)
    tiny = float(np.rad2deg(1e-9))
    edge = PITCH_MAX_DEG - 1e-6      # "pitch error +-80 degrees", with room for the rounding of q2
    named = [("identity", (0, 0, 0)), ("identity", (0, 0, 0)),
             ("tiny-yaw", (tiny, 0, 0)), ("tiny-pitch", (0, -tiny, 0)), ("tiny-roll", (0, 0, tiny)), ("tiny-all", (-tiny, tiny, -tiny)),
             ("yaw+170", (170, 3, -5)), ("yaw-170", (-170, -2, 4)), ("yaw+170-only", (170, 0, 0)), ("yaw-170-pitch", (-170, 40, 10)),
             ("pitch+80", (5, edge, -3)), ("pitch-80", (-8, -edge, 6)), ("pitch+80-only", (0, edge, 0)), ("pitch-80-yaw", (120, -edge, -60)),
             ("roll+179", (2, -4, 179)), ("roll-179", (-3, 5, -179)), ("roll+179-only", (0, 0, 179)), ("roll-179-pitch", (30, -50, -179)),
             ("all-extreme", (170, edge, 179)), ("all-extreme-neg", (-170, -edge, -179)), ("yaw170-roll179", (170, 10, -179)), ("quarter-turns", (90, 0, 90))]
    cases = []
    k = 0
    for tag, err in named:
        cases.append(case(rng, err, rng.uniform(0.1, 1.5), REFERENCE_GAINS if k % 3 else OTHER_GAINS, flip_obs=bool(k % 2), tag=tag))
        k += 1
    cases.append(case(rng, (0, 0, 0), 1.0, REFERENCE_GAINS, False, identity_poses=True, tag="identity-poses"))
    cases.append(case(rng, (20, -10, 30), 0.7, REFERENCE_GAINS, True, identity_poses=True, tag="identity-poses-error"))
    for _ in range(36):
        err = (rng.uniform(-170, 170), rng.uniform(-edge, edge), rng.uniform(-179, 179))
        cases.append(case(rng, err, rng.uniform(0.1, 1.5), REFERENCE_GAINS if k % 3 else OTHER_GAINS, flip_obs=bool(k % 2), tag="random"))
        k += 1
    out = dict(note="generated by tests/golden/make_ypr_goldens.py (mpmath, 50 digits); see its docstring", pitch_max_deg=PITCH_MAX_DEG, cases=cases)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ypr_goldens.json")
    with open(path, "w") as fh:
        json.dump(out, fh)
    print("wrote", path, "cases:", len(cases), "bytes:", os.path.getsize(path))


if __name__ == "__main__":
    main()
