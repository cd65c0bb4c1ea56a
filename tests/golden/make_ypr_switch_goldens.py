#!/usr/bin/env python3
"""Generates tests/golden/ypr_switch_goldens.json — the pin for the switchable yaw/pitch/roll-weighted edge (reference FourDOFErrorWithSwitchingConstraints,
src/CeresResidues.h:338-422; R2ypr, src/utils/PoseManipUtils.cpp:143-158), which the oracle cannot evaluate.

As tests/golden/make_ypr_goldens.py does for FourDOFError, and with its helpers and those of tests/golden/make_functor_goldens.py:
  * residuals: what the functor's operator() computes — [delta_t ; g_y yaw ; g_p pitch ; g_r roll ; 1 - s] in degrees, all seven rows times s, the weight ignored
    (CeresResidues.h:382-397) — in 50 significant digits;
  * Jacobians: 50-digit central differences through the Ceres `EigenQuaternionParameterization::Plus` retraction, step 1e-20, for both poses and the switch.
Nothing here knows the closed-form blocks of csrc/pgo_device_math.hpp, csrc/pgo_sparse_graph_math.hpp or tests/ypr_model.py.

The cases are built as the yaw/pitch/roll generator builds its own: from a wanted error (yaw, pitch, roll), q2 = q1 (x) q_o (x) q_err*.  Conditions, asserted below: every
case has |pitch error| <= 80 degrees (the Euler singularity at 90 degrees is the reference functor's own); yaw to 170, roll to 179 degrees; both signs of q_o; s in
[0.05, 1.2].  40 cases.

Run:  python tests/golden/make_ypr_switch_goldens.py      (deterministic; numpy seed 20261021)
"""
import json
import os
import sys

import mpmath as mp
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_functor_goldens import fl, make_T, mat_to_quat_eigen, mpv, num_jac, plus, qconj, qmul, rand_unit_quat, rotmat  # noqa: E402
from make_ypr_goldens import OTHER_GAINS, PITCH_MAX_DEG, REFERENCE_GAINS, euler_quat, qmul_np, r2ypr_deg, res_ypr  # noqa: E402

mp.mp.dps = 50
S_MIN, S_MAX = 0.05, 1.2


def res_switch_ypr(q1, t1, q2, t2, s, qo, to, g):
    r6 = res_ypr(q1, t1, q2, t2, qo, to, mp.mpf(1), g)
    return [s * x for x in r6] + [s * (1 - s)]


def case(rng, err_deg, s, g, flip_obs, tag):
    assert S_MIN <= s <= S_MAX, (tag, s)
    y, p, r = np.deg2rad(err_deg)
    q_err = euler_quat(y, p, r)
    q1, qo = rand_unit_quat(rng), rand_unit_quat(rng)
    t1, to = rng.normal(size=3) * 5, rng.normal(size=3) * 2
    T16 = make_T(qo, to)
    Tm = mp.matrix(3, 3)
    for c in range(3):
        for rr in range(3):
            Tm[rr, c] = mp.mpf(float(T16[c * 4 + rr]))
    q_obs = np.array([float(x) for x in mat_to_quat_eigen(Tm)])      # the observation the edge record holds: Eigen's quaternion of T's rotation block ...
    if flip_obs:
        q_obs = -q_obs                                              # ... or its negative (the same rotation)
    q2 = qmul_np(qmul_np(q1, q_obs), q_err * np.array([-1, -1, -1, 1.0]))
    q2 = q2 / np.linalg.norm(q2)
    t2 = t1 + rng.normal(size=3) * 2
    Q1, T1, Q2, T2, QO, TO, S0, G = mpv(q1), mpv(t1), mpv(q2), mpv(t2), mpv(q_obs), mpv(to), mp.mpf(float(s)), mpv(g)

    def f(pp):
        a1 = pp.get("th1", [0, 0, 0]); b1 = pp.get("p1", [0, 0, 0]); a2 = pp.get("th2", [0, 0, 0]); b2 = pp.get("p2", [0, 0, 0]); ds = pp.get("s", [0])
        return res_switch_ypr(plus(Q1, a1), [T1[i] + b1[i] for i in range(3)], plus(Q2, a2), [T2[i] + b2[i] for i in range(3)], S0 + ds[0], QO, TO, G)
    res = f({})
    ypr = r2ypr_deg(rotmat(qmul(qmul(qconj(Q2), Q1), QO)))
    assert abs(ypr[1]) <= PITCH_MAX_DEG, (tag, err_deg, float(ypr[1]))
    assert abs(ypr[0]) <= 170 + 1e-6 and abs(ypr[2]) <= 179 + 1e-6, (tag, err_deg)
    J = num_jac(f, 7, [("th1", 3), ("p1", 3), ("th2", 3), ("p2", 3), ("s", 1)])
    J1 = [J["th1"][i] + J["p1"][i] for i in range(7)]
    J2 = [J["th2"][i] + J["p2"][i] for i in range(7)]
    Js = [J["s"][i][0] for i in range(7)]
    return dict(tag=tag, q1=fl(list(q1)), t1=fl(list(t1)), q2=fl(list(q2)), t2=fl(list(t2)), T=fl(list(T16)), q_obs=fl(list(q_obs)), t_obs=fl(list(to)), s=float(s),
                gains=[float(x) for x in g], ypr_deg=fl(ypr), r=fl(res), J1=fl(J1), J2=fl(J2), Js=fl(Js))


def main():
    rng = np.random.default_rng(20261021)
    tiny = float(np.rad2deg(1e-9))
    edge = PITCH_MAX_DEG - 1e-6      # "pitch error +-80 degrees", with room for the rounding of q2
    named = [("identity", (0, 0, 0), 0.99), ("identity-s1", (0, 0, 0), 1.0), ("tiny-all", (-tiny, tiny, -tiny), 0.5),
             ("yaw+170", (170, 3, -5), 0.99), ("yaw-170", (-170, -2, 4), 0.3), ("pitch+80", (5, edge, -3), 0.8), ("pitch-80", (-8, -edge, 6), 1.1),
             ("roll+179", (2, -4, 179), 0.6), ("roll-179", (-3, 5, -179), 0.99), ("all-extreme", (170, edge, 179), S_MIN), ("all-extreme-neg", (-170, -edge, -179), S_MAX),
             ("quarter-turns", (90, 0, 90), 0.7)]
    cases = []
    k = 0
    for tag, err, s in named:
        cases.append(case(rng, err, s, REFERENCE_GAINS if k % 3 else OTHER_GAINS, flip_obs=bool(k % 2), tag=tag))
        k += 1
    while len(cases) < 40:
        err = (rng.uniform(-170, 170), rng.uniform(-edge, edge), rng.uniform(-179, 179))
        cases.append(case(rng, err, rng.uniform(S_MIN, S_MAX), REFERENCE_GAINS if k % 3 else OTHER_GAINS, flip_obs=bool(k % 2), tag="random"))
        k += 1
    out = dict(note="generated by tests/golden/make_ypr_switch_goldens.py (mpmath, 50 digits); see its docstring", pitch_max_deg=PITCH_MAX_DEG, s_range=[S_MIN, S_MAX], cases=cases)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ypr_switch_goldens.json")
    with open(path, "w") as fh:
        json.dump(out, fh)
    print("wrote", path, "cases:", len(cases), "bytes:", os.path.getsize(path))


if __name__ == "__main__":
    main()
