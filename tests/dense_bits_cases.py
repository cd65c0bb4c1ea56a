"""The calls whose returned bits tests/golden/dense_kernel_bits.json records: what scripts/record_dense_kernel_bits.py (which writes the file) and
tests/test_gpu_dense_bits.py (which compares against it) share.  The two paths of libpgo.so whose fp64 MFMA kernels have no recorded bits elsewhere (the dense
covariances have tests/golden/pose_covariance_bits.json), through the hooks Problem.dense_spd_solve and Problem.dense_spd_inverse, at the smallest orders that take
each path:

  solve_64       one tile: dc_first_block_kernel and the sweeps only, no panel or update launch;
  solve_66       padded to 128: one dc_panel_kernel, and one dc_update_kernel that factors the next block ahead;
  solve_200      four tiles: an update grid with tiles off the diagonal, and the skipped quadrant above the diagonal;
  inverse_66     gj_step_kernel (one launch per block step), padded to 128: four steps;
  inverse_200    gj_step_kernel, padded to 256: eight steps, with rows before the pivot, columns beyond it, next_cols and next_rows all occurring;
  inverse_2048   the one order below 2560 that launch_coarse_invert sends down the two-launch path (gj_panels_kernel + gj_update_kernel).

Inputs: A = B B^T + n I with B an n x 8 matrix of integers in [-3, 3], formed in int64 — every entry is an exact small integer, so every host builds the same doubles
whatever sums them; the right-hand side of a solve: integers in [-3, 3].  run(name) returns (inputs, outputs): a list of arrays and a dict of arrays; digests(name)
their sha256."""
import hashlib

import numpy as np

from solve_keyframe_pose_graph_amd import capi

SOLVE_ORDERS = (64, 66, 200)
INVERSE_ORDERS = (66, 200, 2048)
CASE_NAMES = tuple(["solve_%d" % n for n in SOLVE_ORDERS] + ["inverse_%d" % n for n in INVERSE_ORDERS])


def spd_integers(n):
    """(A, b): B B^T + n I and a right-hand side, all entries exact integers"""
    rng = np.random.default_rng(n)
    B = rng.integers(-3, 4, (n, 8), dtype=np.int64)
    A = B @ B.T + n * np.eye(n, dtype=np.int64)
    return np.ascontiguousarray(A.astype(np.float64)), rng.integers(-3, 4, n).astype(np.float64)


def run(name):
    kind, _, order = name.partition("_")
    A, b = spd_integers(int(order))
    P = capi.Problem()
    try:
        if kind == "solve":
            x, _ = P.dense_spd_solve(A, b)
            return [A, b], {"x": x}
        inv, _ = P.dense_spd_inverse(A)
        return [A], {"inverse": inv}
    finally:
        P.close()


def sha(arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(("%s %s\0" % (a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def digests(name):
    """{"inputs": sha256 of the input bytes, "outputs": {name: sha256 of that output's bytes}}"""
    inputs, outputs = run(name)
    return {"inputs": sha(inputs), "outputs": {k: sha([v]) for k, v in sorted(outputs.items())}}
