#!/usr/bin/env python3
"""Generates tests/golden/yaw_goldens.json — the pin for the 4-DoF edge (reference QinFourDOFWeightError, src/CeresResidues.h:426-546, with NormalizeAngle and
YawPitchRollToRotationMatrix of the same file), which the oracle cannot evaluate.

Written from the formulas, as tests/golden/make_ypr_goldens.py is:
  * residuals: what the functor's operator() computes, in 50 significant digits, on the doubles the case holds —
        R_i = Rz(psi_i) Ry(pitch_i) Rx(roll_i) in degrees,  r[0..2] = w (R_i^T (t_j - t_i) - t_meas),  r[3] = w N(psi_j - psi_i - rel_yaw) / 10,
    N = NormalizeAngle: ONE conditional fold by 360 (180 stays 180, 400 becomes 40, 800 becomes 440);
  * Jacobians: 50-digit differences, step 1e-25, in the tangent [psi, t] of either keyframe (the parameterisation adds its delta: its Jacobian is 1).  Where the forward and
    the backward difference agree they are averaged; at a fold of N (yaw argument exactly +-180) they differ by 360 / step, and the one on the side where N is continuous
    is taken — the derivative "wherever N is differentiable" that Ceres' Jets propagate.
Nothing here knows the closed-form blocks of csrc/pgo_sparse_yaw_math.hpp or tests/yaw_model.py.

Cases: 60 random edges (poses to +-5 m, pitch and roll to +-60 degrees, yaws and the relative yaw over the whole circle, weights 1 or in [0.5, 2]) and the hand-made ones:
the yaw argument at 179.9, 180, 180.1, -180, -180.1, 400 and 800 (psi_i = rel_yaw = 0, so that the argument is exactly psi_j in doubles), psi_i at 0 and +-90, t_j = t_i.

Run:  python tests/golden/make_yaw_goldens.py      (deterministic; numpy seed 20261021)
"""
import json
import os

import mpmath as mp
import numpy as np

mp.mp.dps = 50
STEP = mp.mpf("1e-25")
ANGLE_MAX_DEG = 60.0


def normalize(a):
    if a > 180:
        return a - 360
    if a < -180:
        return a + 360
    return a


def rotation(yaw, pitch, roll):
    y, p, r = [x / 180 * mp.pi for x in (yaw, pitch, roll)]
    cy, sy, cp, sp, cr, sr = mp.cos(y), mp.sin(y), mp.cos(p), mp.sin(p), mp.cos(r), mp.sin(r)
    return [[cy * cp, -sy * cr + cy * sp * sr, sy * sr + cy * sp * cr],
            [sy * cp, cy * cr + sy * sp * sr, -cy * sr + sy * sp * cr],
            [-sp, cp * sr, cp * cr]]


def residual(xi, xj, rec):
    """xi, xj = [psi, t0, t1, t2]; rec = [t_meas(3), rel_yaw, pitch_i, roll_i, w]"""
    R = rotation(xi[0], rec[4], rec[5])
    d = [xj[1 + k] - xi[1 + k] for k in range(3)]
    w = rec[6]
    out = [(sum(R[b][a] * d[b] for b in range(3)) - rec[a]) * w for a in range(3)]
    out.append(normalize(xj[0] - xi[0] - rec[3]) * w / 10)
    return out


def jacobian(f, x):
    """4 x 4: d f / d x[k] by differences of step STEP, on the continuous side at a fold"""
    J = [[None] * 4 for _ in range(4)]
    f0 = f(x)
    for k in range(4):
        up, dn = list(x), list(x)
        up[k] += STEP; dn[k] -= STEP
        fu, fd = f(up), f(dn)
        for i in range(4):
            a, b = (fu[i] - f0[i]) / STEP, (f0[i] - fd[i]) / STEP
            J[i][k] = (a + b) / 2 if abs(a - b) <= mp.mpf("1e-15") else (a if abs(a) < abs(b) else b)
    return J


def fl(x):
    return [fl(v) for v in x] if isinstance(x, (list, tuple)) else float(x)


def case(tag, psi_i, t_i, psi_j, t_j, t_meas, rel_yaw, pitch, roll, w):
    xi = [float(psi_i)] + [float(v) for v in t_i]
    xj = [float(psi_j)] + [float(v) for v in t_j]
    rec = [float(v) for v in t_meas] + [float(rel_yaw), float(pitch), float(roll), float(w)]
    assert abs(rec[4]) <= ANGLE_MAX_DEG and abs(rec[5]) <= ANGLE_MAX_DEG and rec[6] > 0
    Xi, Xj, Rec = [mp.mpf(v) for v in xi], [mp.mpf(v) for v in xj], [mp.mpf(v) for v in rec]
    r = residual(Xi, Xj, Rec)
    J1 = jacobian(lambda x: residual(x, Xj, Rec), Xi)
    J2 = jacobian(lambda x: residual(Xi, x, Rec), Xj)
    arg = Xj[0] - Xi[0] - Rec[3]
    return dict(tag=tag, xi=xi, xj=xj, rec=rec, yaw_argument=float(arg), r=fl(r), J1=fl(J1), J2=fl(J2))


def main():
    rng = np.random.default_rng(20261021)

    def rand(tag, psi_i=None, psi_j=None, rel_yaw=None, same_t=False, w=None):
        t_i = rng.normal(size=3) * 5
        t_j = t_i.copy() if same_t else t_i + rng.normal(size=3) * 2
        return case(tag, rng.uniform(-180, 180) if psi_i is None else psi_i, t_i, rng.uniform(-180, 180) if psi_j is None else psi_j, t_j, rng.normal(size=3) * 2,
                    rng.uniform(-180, 180) if rel_yaw is None else rel_yaw, rng.uniform(-ANGLE_MAX_DEG, ANGLE_MAX_DEG), rng.uniform(-ANGLE_MAX_DEG, ANGLE_MAX_DEG),
                    1.0 if w is None else w)
    cases = []
    for a in (179.9, 180.0, 180.1, -180.0, -180.1, 400.0, 800.0):
        cases.append(rand("argument%+g" % a, psi_i=0.0, psi_j=a, rel_yaw=0.0))
    cases.append(rand("argument+180-by-difference", psi_i=10.0, psi_j=-150.0, rel_yaw=20.0 - 360.0 + 0.0))      # -150 - 10 + 340 = 180 exactly
    for a in (0.0, 90.0, -90.0):
        cases.append(rand("psi_i%+g" % a, psi_i=a))
    cases.append(rand("same-t", same_t=True))
    cases.append(rand("same-t-psi_i-0", psi_i=0.0, same_t=True, w=1.5))
    for k in range(60):
        cases.append(rand("random", w=None if k % 3 else rng.uniform(0.5, 2.0)))
    assert [c["yaw_argument"] for c in cases[:8]] == [179.9, 180.0, 180.1, -180.0, -180.1, 400.0, 800.0, 180.0]
    folded = [179.9, 180.0, 180.1 - 360.0, -180.0, 360.0 - 180.1, 40.0, 440.0, 180.0]
    assert all(abs(c["r"][3] * 10 - v) <= 1e-12 for c, v in zip(cases[:8], folded))
    args = [c["yaw_argument"] for c in cases[13:]]
    assert min(args) < -360 and max(args) > 360 and any(abs(a) < 180 for a in args)      # both folds and the middle among the random ones
    out = dict(note="generated by tests/golden/make_yaw_goldens.py (mpmath, 50 digits); see its docstring", angle_max_deg=ANGLE_MAX_DEG, cases=cases)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "yaw_goldens.json")
    with open(path, "w") as fh:
        json.dump(out, fh)
    print("wrote", path, "cases:", len(cases), "bytes:", os.path.getsize(path))


if __name__ == "__main__":
    main()
