"""The yaw/pitch/roll-weighted relative-pose edge (reference FourDOFError, src/CeresResidues.h:252-333, with R2ypr of src/utils/PoseManipUtils.cpp:143-158) in float64 numpy:
the residual from the reference's formulas and the Jacobian blocks from the closed form of DESIGN.md (left perturbation q <- (d, 1) (x) q, tangent order [dtheta, dt]).
A yardstick for these edges, which the oracle cannot evaluate; itself pinned against 50-digit goldens by tests/test_ypr_host.py."""
import numpy as np

DEG = 180.0 / np.pi
REFERENCE_GAINS = (4.0, 10.0, 10.0)


def rot(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz])


def skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])


def mat_to_quat(R):
    """a unit quaternion (x, y, z, w) of R.  Its sign is free: the residual below depends on R(delta_q) alone"""
    t = np.trace(R)
    if t > 0:
        s = np.sqrt(t + 1.0) * 2
        return np.array([(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, 0.25 * s])
    i = int(np.argmax(np.diag(R)))
    j, k = (i + 1) % 3, (i + 2) % 3
    s = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0) * 2
    q = np.zeros(4)
    q[i] = 0.25 * s
    q[3] = (R[k, j] - R[j, k]) / s
    q[j] = (R[j, i] + R[i, j]) / s
    q[k] = (R[k, i] + R[i, k]) / s
    return q


def obs_of(T16):
    T = np.asarray(T16, dtype=np.float64).reshape(4, 4).T
    return mat_to_quat(T[:3, :3]), T[:3, 3].copy()


def edge(q1, t1, q2, t2, qo, to, w, g, want_blocks=True):
    """r[6], J1[6, 6], J2[6, 6], (yaw, pitch, roll) in degrees"""
    q1, t1, q2, t2, qo, to, g = (np.asarray(x, dtype=np.float64) for x in (q1, t1, q2, t2, qo, to, g))
    R1, R2 = rot(q1), rot(q2)
    a = R1 @ to
    v = t1 + a - t2
    dt = R2.T @ v
    R = rot(qmul(qmul(q2 * np.array([-1, -1, -1, 1.0]), q1), qo))
    y = np.arctan2(R[1, 0], R[0, 0])
    cy, sy = np.cos(y), np.sin(y)
    p = np.arctan2(-R[2, 0], R[0, 0] * cy + R[1, 0] * sy)
    r = np.arctan2(R[0, 2] * sy - R[1, 2] * cy, -R[0, 1] * sy + R[1, 1] * cy)
    ypr = np.array([y, p, r]) * DEG
    res = w * np.concatenate([dt, g * ypr])
    if not want_blocks:
        return res, None, None, ypr
    h = np.hypot(R[0, 0], R[1, 0])
    sp = -R[2, 0]
    E = np.array([[sp * cy / h, sp * sy / h, 1.0], [-sy, cy, 0.0], [cy / h, sy / h, 0.0]])
    Mp = (g * DEG)[:, None] * (E @ R2.T)
    J1, J2 = np.zeros((6, 6)), np.zeros((6, 6))
    J1[:3, :3] = -2 * w * R2.T @ skew(a)
    J1[:3, 3:] = w * R2.T
    J2[:3, :3] = 2 * w * R2.T @ skew(v)
    J2[:3, 3:] = -w * R2.T
    J1[3:, :3] = 2 * w * Mp
    J2[3:, :3] = -2 * w * Mp
    return res, J1, J2, ypr


def rho_c(loss, s):
    """rho(s) and c = sqrt(rho'(s)) of ceres::HuberLoss(a) / ceres::CauchyLoss(a); loss None: trivial"""
    if loss is None:
        return s, 1.0
    kind, a = loss
    b = a * a
    if kind == "huber":
        return (s, 1.0) if s <= b else (2.0 * a * np.sqrt(s) - b, np.sqrt(a / np.sqrt(s)))
    u = 1.0 + s / b
    return b * np.log(u), np.sqrt(1.0 / u)
