"""The requests whose returned bits tests/golden/pose_covariance_bits.json records: what scripts/record_pose_covariance_bits.py (which writes the file) and
tests/test_gpu_dense_covariance.py (which compares against it) share.  Pose blocks only, on the smallest inputs at which the covariance launches take each of their
paths:

  spd66, spd200, spd204   the kernels alone (dense_spd_covariance) on exact matrices, see spd();
  loops24_csr, _dense     param_cov_ref.with_loops(24, LOOPS): three tiles, keyframe 10 across a tile edge, switchable loop closures in the Schur complement; the
                          block-CSR PCG's handle and the dense solver's;
  tl200_constant          tl200 with keyframes 20-29 constant: identity rows and zero blocks in mid-matrix, 19 tiles.

run(name) returns the blocks of one case, (n_pairs, 6, 6); for the loops24 cases also what covariance() returns for the same pairs."""
import numpy as np

from solve_keyframe_pose_graph_amd import capi
from tests import param_cov_ref as pref
from tests import precond_cases as pc
from tests import util

LOOPS = [(10, 11), (0, 23), (23, 0), (5, 15), (15, 5), (7, 9), (9, 7)]      # as tests/test_gpu_param_covariance.py
POSE_PAIRS_24 = [(0, 0), (23, 23), (10, 10), (0, 23), (10, 10), (1, 22), (22, 1), (11, 10)]
CONSTANT = tuple(range(20, 30))


def node_pairs(first, last, mid):
    return [(first, first), (last, last), (mid, mid), (first, last), (mid, mid), (first + 1, last - 1), (last - 1, first + 1)]


def spd(n):
    """B B^T + n I with the integer entries of B in [-3, 3] from the linear congruential generator x <- (1664525 x + 1013904223) mod 2^32 (x0 = n; the entry is
    (x >> 16) mod 7 - 3, row by row): every entry is a small integer, so the matrix is the same doubles wherever it is built"""
    x = n
    B = np.zeros((n, n))
    for i in range(n):
        for j in range(n):
            x = (1664525 * x + 1013904223) % (1 << 32)
            B[i, j] = (x >> 16) % 7 - 3
    return B @ B.T + n * np.eye(n)


# name -> (order, pairs).  66: padding, 11 nodes, node 10 across the tile edge, every pair.  200: 33 nodes and two rows that belong to none; node 32 begins the fourth
# tile, so the zero skipping of the pair (32, 32) starts there; (20, 21) lies across the edge at 128.  204: the same with node 33 (rows 198-203) in mid-tile.
KERNEL_CASES = {
    "spd66": (66, [(a, b) for a in range(11) for b in range(11)]),
    "spd200": (200, [(32, 32), (0, 32), (20, 21)]),
    "spd204": (204, [(33, 33), (0, 33), (20, 21)]),
}
HANDLE_CASES = ("loops24_csr", "loops24_dense", "tl200_constant")
CASES = tuple(KERNEL_CASES) + HANDLE_CASES


def run(name):
    """{"pose": blocks} and, for the loops24 cases, {"covariance": the same pairs through covariance()}"""
    if name in KERNEL_CASES:
        n, pairs = KERNEL_CASES[name]
        P = capi.Problem()
        cov, _ = P.dense_spd_covariance(spd(n), pairs)
        P.close()
        return {"pose": cov}
    if name == "tl200_constant":
        g = pc.graph("tl200")
        q, t, s = pc.state(g)
        P = util.pgo_problem(g, True, linear_solver=capi.LINEAR_PCG_BLOCK_JACOBI)
        P.set_nodes_constant(np.asarray(CONSTANT, dtype=np.int32))
        cov = P.pose_covariance(q, t, s, node_pairs(0, 199, 10))
        P.close()
        return {"pose": cov}
    g = pref.with_loops(24, LOOPS)
    q, t, s = pc.state(g)
    P = util.pgo_problem(g, True, linear_solver={"loops24_csr": capi.LINEAR_PCG_BLOCK_JACOBI, "loops24_dense": capi.LINEAR_DENSE_CHOLESKY}[name])
    cov = P.pose_covariance(q, t, s, POSE_PAIRS_24)
    par = np.stack(P.covariance(q, t, s, POSE_PAIRS_24))
    P.close()
    return {"pose": cov, "covariance": par}
