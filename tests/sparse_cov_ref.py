"""Reference for covariance blocks on graphs above the dense limit (tests/test_gpu_sparse_cholesky.py): the requested columns of S^-1 without a dense matrix.

S, the undamped Schur complement over the keyframes' 6 N coordinates (identity on the keyframes outside the system), is assembled here from the handle's normal
blocks — independently of pgo_sparse_reduce_normal_blocks — as a sparse matrix, every entry summed in np.longdouble.  The columns Z = S^-1 V^T of the requested row
groups V (a keyframe: six unit rows; a switch e: the row -c_e / h_e) are solved by scipy.sparse.linalg.splu and refined with np.longdouble residuals over the CSR data
until the residual stops falling: tests/dense_cov_ref.py's refined_columns on a sparse matrix.  The blocks are V_a Z_b, plus 1 / h_e for a switch with itself.

e_np is plain fp64 on the same normal blocks: S summed in fp64 by scipy, one splu solve, no refinement.  Error measure and MARGIN: tests/dense_cov_ref.py's."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from tests.dense_cov_ref import MARGIN


def schur_triplets(N, free, in_system, diag, off, c, hss, rel_c1, rel_c2, sw_c1, sw_c2):
    """(rows, cols, values in np.longdouble) of S with duplicates, lower and upper triangle; identity on the keyframes outside the system"""
    L = np.longdouble
    k6 = np.arange(6)
    R, Cc, V = [], [], []

    def add(a, b, blk):
        r, cidx = np.meshgrid(6 * a + k6, 6 * b + k6, indexing="ij")
        R.append(r.reshape(-1)); Cc.append(cidx.reshape(-1)); V.append(np.asarray(blk, dtype=L).reshape(-1))

    for i in range(N):
        add(i, i, diag[i] if in_system[i] else np.eye(6))
    E = len(rel_c1)
    ends = [(int(a), int(b), off[e], None) for e, (a, b) in enumerate(zip(rel_c1, rel_c2))] + [(int(a), int(b), off[E + e], e) for e, (a, b) in enumerate(zip(sw_c1, sw_c2))]
    for a, b, blk, s in ends:
        if s is not None:
            ca, cb, h = c[s, :6].astype(L), c[s, 6:].astype(L), L(hss[s])
            if free[a]:
                add(a, a, -np.outer(ca, ca) / h)
            if free[b]:
                add(b, b, -np.outer(cb, cb) / h)
        if a == b or not (free[a] and free[b]):
            continue
        full = blk.astype(L) if s is None else blk.astype(L) - np.outer(ca, cb) / h
        add(a, b, full); add(b, a, full.T)
    return np.concatenate(R), np.concatenate(Cc), np.concatenate(V)


def summed_csr(n, rows, cols, vals):
    """(indptr, indices, data): duplicates summed in the precision of vals, rows and columns ascending"""
    key = rows.astype(np.int64) * n + cols
    order = np.argsort(key, kind="stable")
    key, vals = key[order], vals[order]
    first = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]]))
    data = np.add.reduceat(vals, first)
    ukey = key[first]
    r, cidx = ukey // n, ukey % n
    indptr = np.zeros(n + 1, np.int64)
    np.add.at(indptr, r + 1, 1)
    return np.cumsum(indptr), cidx.astype(np.int64), data


def csr_residual(indptr, indices, data, X, E):
    """E - S X in np.longdouble, column by column"""
    out = np.empty_like(E)
    nonempty = indptr[:-1] < indptr[1:]      # (every row has its diagonal entry)
    assert nonempty.all()
    for j in range(X.shape[1]):
        out[:, j] = E[:, j] - np.add.reduceat(data * X[indices, j], indptr[:-1])
    return out


class Reference:
    """reference and plain-fp64 blocks of `pairs` (block ids: keyframe a, or N + switch index; the switchable edges' switch indices are their positions)"""

    def __init__(self, N, free, in_system, normal_blocks, rel_c1, rel_c2, sw_c1, sw_c2, pairs):
        diag, _, off, c, hss, _ = normal_blocks
        L = np.longdouble
        n = 6 * N
        self.pairs = [(int(a), int(b)) for a, b in pairs]
        self.hss = hss
        self.N = N
        ids = sorted({i for p in self.pairs for i in p})
        self.at, cols = {}, []
        for i in ids:
            if i < N:
                v = np.zeros((n, 6), L); v[6 * i + np.arange(6), np.arange(6)] = 1.0
            else:
                e = i - N
                v = np.zeros((n, 1), L)
                for side, node in enumerate((int(sw_c1[e]), int(sw_c2[e]))):
                    if free[node]:
                        v[6 * node:6 * node + 6, 0] += -c[e, 6 * side:6 * side + 6].astype(L) / L(hss[e])
            self.at[i] = np.arange(len(cols), len(cols) + v.shape[1])
            cols.extend(v.T)
        V = np.stack(cols, axis=1)                                   # n x m, np.longdouble
        rows, cidx, vals = schur_triplets(N, free, in_system, diag, off, c, hss, rel_c1, rel_c2, sw_c1, sw_c2)
        keep = cidx <= rows                                          # the lower triangle, mirrored: what the factorisation is given
        rows, cidx, vals = rows[keep], cidx[keep], vals[keep]
        strict = cidx < rows
        rows, cidx, vals = np.concatenate([rows, cidx[strict]]), np.concatenate([cidx, rows[strict]]), np.concatenate([vals, vals[strict]])
        indptr, indices, data = summed_csr(n, rows, cidx, vals)
        S_ref = sp.csr_matrix((data.astype(np.float64), indices, indptr), shape=(n, n))
        S_np = sp.coo_matrix((vals.astype(np.float64), (rows, cidx)), shape=(n, n)).tocsc()      # duplicates summed in fp64
        self.nnz = S_ref.nnz
        lu = spla.splu(S_ref.tocsc())
        X = lu.solve(V.astype(np.float64)).astype(L)
        best, keepX, self.refinements = np.inf, X, 0
        for _ in range(20):
            Rr = csr_residual(indptr, indices, data, X, V)
            r = float(np.abs(Rr).max())
            if not r < best:
                break
            best, keepX = r, X
            X = X + lu.solve(Rr.astype(np.float64)).astype(L)
            self.refinements += 1
        self.residual = best
        self.V = V
        self.G = V.T @ keepX                                         # m x m: every block between the requested ids
        self.var = np.array([float(self._block(self.G, i, i)[k, k]) for i in ids for k in range(len(self.at[i]))])
        self.var_at = {i: self.var[self.at[i]] for i in ids}
        Xnp = spla.splu(S_np).solve(V.astype(np.float64))
        self.e_np = self.error([self._block(V.astype(np.float64).T @ Xnp, a, b).astype(np.float64) for a, b in self.pairs])
        self.bound = MARGIN * self.e_np

    def _block(self, G, a, b):
        blk = G[np.ix_(self.at[a], self.at[b])]
        if a == b and a >= self.N:
            blk = blk + type(blk[0, 0])(1.0) / type(blk[0, 0])(self.hss[a - self.N])
        return blk

    def blocks(self):
        return [self._block(self.G, a, b).astype(np.float64) for a, b in self.pairs]

    def error(self, cov):
        worst = 0.0
        for (a, b), blk in zip(self.pairs, cov):
            d = np.abs(np.asarray(blk).astype(np.longdouble) - self._block(self.G, a, b))
            worst = max(worst, float((d / np.sqrt(np.outer(self.var_at[a], self.var_at[b]))).max()))
        return worst
