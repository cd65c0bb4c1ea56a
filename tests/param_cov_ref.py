"""What tests/test_param_cov_host.py (CPU) and tests/test_gpu_param_covariance.py (GPU) share: the reference for covariance blocks of pose AND switch parameters, the
graphs with hand-placed loop closures, and the handle's FULL normal matrix.

Reference.  The code under test factors the Schur complement S and marginalises the switches by algebra (csrc/pgo_dense_math.hpp).  The reference never forms S: it is
the inverse of the full matrix H = [H_pp C; C^T diag(h)] over the pose entries and the switches, refined in np.longdouble as tests/dense_cov_ref.py refines — an
independent check of the marginalisation.  e_np is plain fp64 numpy on the same full matrix (Cholesky factor, triangular inverse, Gram product); the code under test
gets MARGIN = 8 x e_np, the convention of tests/dense_cov_ref.py.  The error measure is that module's scaled entrywise e, the variances extended to the switch entries."""
import dataclasses

import numpy as np
import scipy.linalg

from tests import dense_cov_ref as ref
from tests import util

MARGIN = ref.MARGIN


def full_matrix(S, sw_node, sw_c, sw_h):
    """H = [S + C diag(h)^-1 C^T, C; C^T, diag(h)] for switch columns in block form (node pair or -1, twelve values, h)"""
    n, ns = S.shape[0], len(sw_h)
    Cs = np.zeros((n, ns))
    for s in range(ns):
        for side in range(2):
            nd = int(sw_node[s][side])
            if nd >= 0:
                Cs[6 * nd:6 * nd + 6, s] = sw_c[s][6 * side:6 * side + 6]
    H = np.zeros((n + ns, n + ns))
    H[:n, :n] = S + (Cs / sw_h) @ Cs.T
    H[:n, n:] = Cs
    H[n:, :n] = Cs.T
    H[n:, n:] = np.diag(sw_h)
    return H


class FullReference:
    """reference blocks and plain-numpy blocks of the requested ids on a full matrix H; rows_of(id) -> the rows of H of block id"""

    def __init__(self, H, pairs, rows_of):
        self.pairs = [(int(a), int(b)) for a, b in pairs]
        ids = sorted({i for p in self.pairs for i in p})
        self.at, cols = {}, []
        for i in ids:
            r = list(rows_of(i))
            self.at[i] = np.arange(len(cols), len(cols) + len(r))
            cols += r
        cols = np.asarray(cols, dtype=np.int64)
        self.S = ref.refined_columns(H, cols)[cols]
        self.var = np.diag(self.S).astype(np.float64)
        Linv = scipy.linalg.solve_triangular(np.linalg.cholesky(H), np.eye(H.shape[0]), lower=True)
        Snp = Linv[:, cols].T @ Linv[:, cols]
        self.e_np = self.error([Snp[np.ix_(self.at[a], self.at[b])] for a, b in self.pairs])
        self.bound = MARGIN * self.e_np

    def blocks(self):
        return [self.S[np.ix_(self.at[a], self.at[b])].astype(np.float64) for a, b in self.pairs]

    def error(self, cov):
        worst = 0.0
        for (a, b), blk in zip(self.pairs, cov):
            ra, rb = self.at[a], self.at[b]
            assert blk.shape == (len(ra), len(rb)), (a, b, blk.shape)
            d = np.abs(blk.astype(np.longdouble) - self.S[np.ix_(ra, rb)])
            worst = max(worst, float((d / np.sqrt(np.outer(self.var[ra], self.var[rb]))).max()))
        return worst


def check_exact_structure(pairs, cov):
    """cov(b, a) == cov(a, b)^T bit for bit wherever both were asked for, a block with itself exactly symmetric, a repeated pair the same bits"""
    seen = {}
    for (a, b), blk in zip(pairs, cov):
        if a == b:
            assert np.array_equal(blk, blk.T), (a, b)
        if (b, a) in seen:
            assert np.array_equal(blk, seen[(b, a)].T), (a, b)
        if (a, b) in seen:
            assert np.array_equal(blk, seen[(a, b)]), (a, b)
        seen[(a, b)] = blk


def spd_case(n, n_sw=9):
    """dense_cov_ref.spd(n) as the Schur complement, and n_sw random switch columns: the first and the last node in both orders, node 10 (rows 60-65 straddle a tile
    edge) where it exists, one side dropped, no side at all, the rest random"""
    rng = np.random.default_rng(1000 + n)
    S = ref.spd(n)
    last = n // 6 - 1
    mid = min(10, last - 1)
    nodes = [(0, last), (last, 0), (mid, mid - 1), (mid - 1, mid), (5, -1), (-1, last - 1), (-1, -1)]
    while len(nodes) < n_sw:
        a, b = rng.choice(last + 1, 2, replace=False)
        nodes.append((int(a), int(b)))
    nodes = np.asarray(nodes[:n_sw], dtype=np.int32)
    c = 0.3 * rng.standard_normal((n_sw, 12))
    h = rng.uniform(0.25, 1.25, n_sw)
    return S, nodes, c, h


def spd_pairs(n, n_sw):
    """ids: node i, or n // 6 + s.  Node-node pairs of dense_cov_ref.spd_pairs, every switch with itself, switch-switch and node-switch pairs in both orders"""
    N = n // 6
    pairs = [(a, b) for a, b in ref.spd_pairs(n)]
    pairs += [(N + s, N + s) for s in range(n_sw)]
    pairs += [(N + 0, N + 1), (N + 1, N + 0), (N + 2, N + 6), (N + 6, N + 2), (N + 4, N + 5)]
    pairs += [(0, N + 0), (N + 0, 0), (N - 1, N + 2), (N + 2, N - 1), (3, N + 6), (N + 6, 3), (2, N + 4), (N + 5, N - 2)]
    return pairs


def spd_rows_of(n):
    N = n // 6
    return lambda i: range(6 * i, 6 * i + 6) if i < N else [n + (i - N)]


# ---- graphs with hand-placed switchable loop closures
def with_loops(n, loops, f=2, seed=11):
    """an odometry chain of n keyframes (util.small_graph finds no loop closure on trajectories this short) with a regulariser on keyframe 0, plus switchable loop
    closures between the given (c1, c2) pairs; their measurements are the true relative poses"""
    g = util.small_graph(n, 0, f=f, seed=seed)
    M = util.poses_to_matrices(g.truth_q, g.truth_t).reshape(-1, 4, 4).transpose(0, 2, 1)
    c1 = np.asarray([a for a, _ in loops], dtype=np.int32); c2 = np.asarray([b for _, b in loops], dtype=np.int32)
    T = np.stack([np.linalg.inv(M[a]) @ M[b] for a, b in loops]) if len(loops) else np.zeros((0, 4, 4))
    T = np.ascontiguousarray(T.transpose(0, 2, 1)).reshape(-1, 16)
    return dataclasses.replace(g, loop_c1=c1, loop_c2=c2, loop_T=T, loop_w=np.ones(len(loops)), loop_is_outlier=np.zeros(len(loops), np.int32))


def handle_full_matrix(P, g, free):
    """(H, rows_of): the full undamped normal matrix over the free keyframes' tangent entries and ALL switches, from the handle's normal blocks at its last linearisation;
    block ids: keyframe a, or n_poses + loop index"""
    N, S = g.n_poses, g.n_loops
    diag, _, off, c, hss, _ = P.normal_blocks()
    H = np.zeros((6 * N + S, 6 * N + S))
    for n in range(N):
        H[6 * n:6 * n + 6, 6 * n:6 * n + 6] = diag[n]
    c1 = np.concatenate([g.odom_c1, g.loop_c1]); c2 = np.concatenate([g.odom_c2, g.loop_c2])
    for e in range(len(off)):
        a, b = int(c1[e]), int(c2[e])
        H[6 * a:6 * a + 6, 6 * b:6 * b + 6] += off[e]
        H[6 * b:6 * b + 6, 6 * a:6 * a + 6] += off[e].T
    for e in range(S):
        a, b = int(g.loop_c1[e]), int(g.loop_c2[e])
        H[6 * a:6 * a + 6, 6 * N + e] = H[6 * N + e, 6 * a:6 * a + 6] = c[e, :6]
        H[6 * b:6 * b + 6, 6 * N + e] = H[6 * N + e, 6 * b:6 * b + 6] = c[e, 6:]
        H[6 * N + e, 6 * N + e] = hss[e]
    keep = np.concatenate([ref.node_columns(np.flatnonzero(free)), 6 * N + np.arange(S)]).astype(np.int64)
    pos = np.cumsum(free) - 1
    nf = 6 * int(free.sum())
    rows_of = lambda i: range(6 * pos[i], 6 * pos[i] + 6) if i < N else [nf + (i - N)]
    return H[np.ix_(keep, keep)], rows_of
