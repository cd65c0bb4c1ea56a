"""numpy model of the 4-DoF edge (reference QinFourDOFWeightError, src/CeresResidues.h:426-546) and of a whole graph of them, written from the functor's text: what
scipy minimises in tests/test_sparse_yaw_host.py, and what the closed forms of csrc/pgo_sparse_yaw_math.hpp are held to beside the 50-digit goldens.  Angles in degrees."""
import numpy as np


def normalize_angle(a):
    """the reference's NormalizeAngle: one conditional fold"""
    a = np.asarray(a, dtype=np.float64)
    return np.where(a > 180.0, a - 360.0, np.where(a < -180.0, a + 360.0, a))


def rotation(yaw, pitch, roll):
    """YawPitchRollToRotationMatrix -> (..., 3, 3)"""
    y, p, r = [np.asarray(x, dtype=np.float64) / 180.0 * np.pi for x in (yaw, pitch, roll)]
    cy, sy, cp, sp, cr, sr = np.cos(y), np.sin(y), np.cos(p), np.sin(p), np.cos(r), np.sin(r)
    rows = [[cy * cp, -sy * cr + cy * sp * sr, sy * sr + cy * sp * cr], [sy * cp, cy * cr + sy * sp * sr, -cy * sr + sy * sp * cr], [-sp + 0 * cy, cp * sr + 0 * cy, cp * cr + 0 * cy]]
    return np.stack([np.stack(row, axis=-1) for row in rows], axis=-2)


def residuals(c1, c2, t_meas, rel_yaw, pitch_i, roll_i, w, yaw, t, smooth_below=None):
    """(E, 4) residuals of the edges at the state (yaw (N,), t (N, 3)).  smooth_below: assert |psi_j - psi_i - rel_yaw| < smooth_below on every edge (no fold anywhere near:
    the problem a smooth minimiser may be given)"""
    R = rotation(yaw[c1], pitch_i, roll_i)
    d = t[c2] - t[c1]
    arg = yaw[c2] - yaw[c1] - rel_yaw
    if smooth_below is not None:
        assert np.abs(arg).max() < smooth_below, np.abs(arg).max()
    r = np.empty((len(c1), 4))
    r[:, :3] = (np.einsum("eba,eb->ea", R, d) - t_meas) * w[:, None]
    r[:, 3] = normalize_angle(arg) * w / 10.0
    return r
