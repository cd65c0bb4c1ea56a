"""What tests/test_dense_cov_host.py (CPU) and tests/test_gpu_dense_covariance.py (GPU) share: the reference covariance, the error measure and the matrices.

Reference.  Sigma_ref = H^-1 refined in np.longdouble by Newton steps X <- X + X0 (I - H X) from numpy's fp64 inverse X0 until the longdouble residual stops falling.
The columns of the iteration decouple, so only the columns of the requested "nodes" (node i = rows 6 i .. 6 i + 5) are carried: the full longdouble products of order
1088 would take minutes in numpy.  e_np is the error of plain fp64 numpy on the same matrix (Cholesky factor, triangular inverse, Gram product) against that reference;
the code under test gets 8 x e_np (the convention of tests/test_gpu_precond_operator.py): the same backward-stable algorithm in another summation order.

Error measure.  e(S, S_ref) = max_ij |S - S_ref|_ij / sqrt(S_ref,ii S_ref,jj): entrywise, scaled by the two variances (the variances of these graphs span 3e-2 .. 7e2: an
unscaled norm would hide the small ones)."""
import numpy as np
import scipy.linalg

MARGIN = 8.0


def spd(n):
    """as tests/test_dense_cholesky_host.py builds them"""
    rng = np.random.default_rng(n)
    B = rng.standard_normal((n, max(8, n // 2)))
    A = B @ B.T + np.diag(rng.uniform(1e-3, 1.0, n))
    return 0.5 * (A + A.T)


def node_columns(nodes):
    return (np.asarray(nodes, dtype=np.int64)[:, None] * 6 + np.arange(6)).reshape(-1)


def refined_columns(H, cols):
    """the columns `cols` of the refined inverse of H, in np.longdouble"""
    Hl = H.astype(np.longdouble)
    X0 = np.linalg.inv(H).astype(np.longdouble)
    E = np.zeros((H.shape[0], len(cols)), np.longdouble)
    E[cols, np.arange(len(cols))] = 1.0
    X = X0[:, cols].copy()
    best = np.inf
    for _ in range(20):
        R = E - Hl @ X
        r = float(np.abs(R).max())
        if not r < best:
            break
        best, keep = r, X
        X = X + X0 @ R
    return keep


class Reference:
    """reference blocks and plain-numpy blocks of the pairs' nodes, for one matrix"""

    def __init__(self, H, pairs):
        self.pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        self.nodes = np.unique(self.pairs)
        cols = node_columns(self.nodes)
        X = refined_columns(H, cols)[cols]                          # the nodes' rows and columns
        self.var = np.diag(X).astype(np.float64)
        self.S = X
        Linv = scipy.linalg.solve_triangular(np.linalg.cholesky(H), np.eye(H.shape[0]), lower=True)
        Snp = Linv[:, cols].T @ Linv[:, cols]
        self.e_np = self.error(np.stack([self._block(Snp, a, b) for a, b in self.pairs]))
        self.bound = MARGIN * self.e_np

    def _at(self, node):
        return 6 * int(np.searchsorted(self.nodes, node))

    def _block(self, X, a, b):
        ra, rb = self._at(a), self._at(b)
        return X[ra:ra + 6, rb:rb + 6]

    def blocks(self):
        return np.stack([self._block(self.S, a, b) for a, b in self.pairs]).astype(np.float64)

    def error(self, cov):
        """e of the (n_pairs, 6, 6) blocks `cov` against the reference"""
        worst = 0.0
        for (a, b), blk in zip(self.pairs, cov):
            ra, rb = self._at(a), self._at(b)
            d = np.abs(blk.astype(np.longdouble) - self.S[ra:ra + 6, rb:rb + 6])
            worst = max(worst, float((d / np.sqrt(np.outer(self.var[ra:ra + 6], self.var[rb:rb + 6]))).max()))
        return worst


def scaled_error(S, S_ref):
    """e for two full matrices"""
    d = np.sqrt(np.diag(S_ref))
    return float((np.abs(S - S_ref) / np.outer(d, d)).max())


def spd_pairs(n):
    """the pairs of the kernel tests on an n x n matrix: first node, last node, node 10 (rows 60-65 straddle the first tile boundary) where it exists, a far off-diagonal
    pair, a repeated node, and (a, b) together with (b, a)"""
    last = n // 6 - 1
    mid = min(10, last)
    return [(0, 0), (last, last), (mid, mid), (0, last), (mid, mid), (1, last - 1), (last - 1, 1)]


def check_exact_structure(pairs, cov):
    """cov(b, a) == cov(a, b)^T bit for bit wherever both were asked for, diagonal blocks exactly symmetric, a repeated pair the same bits"""
    seen = {}
    for (a, b), blk in zip(pairs, cov):
        if a == b:
            assert np.array_equal(blk, blk.T), (a, b)
        if (b, a) in seen:
            assert np.array_equal(blk, seen[(b, a)].T), (a, b)
        if (a, b) in seen:
            assert np.array_equal(blk, seen[(a, b)]), (a, b)
        seen[(a, b)] = blk


def handle_matrix(P, g, switchable, free):
    """the undamped Schur complement over the free keyframes, from the handle's normal blocks at its last linearisation (the K2 parity hook): what the factorisation is
    given, formed on the host.  Only the lower triangle of the pose part is used, as by the factorisation."""
    N = g.n_poses
    S = g.n_loops if switchable else 0
    diag, _, off, c, hss, _ = P.normal_blocks()
    H = np.zeros((6 * N, 6 * N))
    for n in range(N):
        H[6 * n:6 * n + 6, 6 * n:6 * n + 6] = diag[n]
    c1 = np.concatenate([g.odom_c1, g.loop_c1]); c2 = np.concatenate([g.odom_c2, g.loop_c2])
    for e in range(len(off)):
        a, b = int(c1[e]), int(c2[e])
        H[6 * a:6 * a + 6, 6 * b:6 * b + 6] += off[e]
        H[6 * b:6 * b + 6, 6 * a:6 * a + 6] += off[e].T
    Cs = np.zeros((6 * N, S))
    for e in range(S):
        a, b = int(g.loop_c1[e]), int(g.loop_c2[e])
        Cs[6 * a:6 * a + 6, e] = c[e, :6]
        Cs[6 * b:6 * b + 6, e] = c[e, 6:]
    A = H - (Cs / hss) @ Cs.T if S else H
    A = np.tril(A) + np.tril(A, -1).T
    rows = node_columns(np.flatnonzero(free))
    return A[np.ix_(rows, rows)]


def referenced(g):
    r = np.zeros(g.n_poses, bool)
    for c in (g.odom_c1, g.odom_c2, g.loop_c1, g.loop_c2, g.reg_node):
        r[np.asarray(c, dtype=np.int64)] = True
    return r
