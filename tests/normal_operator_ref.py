"""An independent fp64 reference of the LM normal operator that scales (numpy and scipy.sparse only): what tests/test_gpu_normal_operator.py compares the matrix-free
and the assembled matvec, K2's per-keyframe sums and the fused PCG forms with, itself checked on the CPU in tests/test_normal_operator_ref.py.

reference()   builds the damped Schur complement EDGE BY EDGE from the checker's per-edge Jacobian blocks (O.jacobian_blocks, kinds 0 / 1 / 2) and residuals: H = sum J^T J
              as 6 x 6 blocks over keyframes plus one scalar per switch, the LM diagonal exactly as tests/precond_model.py::Linearisation.system takes it
              (scale = 1 / (1 + sqrt(diag H)), lambda = clip(scale^2 diag H, 1e-6, 1e32) / radius / scale^2), every switch eliminated by its own edge's rank-one term.
              The result is a scipy.sparse matrix of 6 N rows at any N and the reduced right-hand side, over ALL keyframes as if every one were free.
device_rows() turns that into what the device's operators define for keyframes outside the system (see its docstring).
tile_rule()   restates the tile-closing rule of pack_mf_tiles (csrc/pgo_graph.hip) so that a case can be shown, on the CPU, to reach the tile condition it is named for.
compare()     the GPU test's comparison of two dense operators; the CPU tests feed it deliberately wrong variants of the reference (`variant`) to show its teeth."""
import numpy as np
import scipy.sparse as sp

MF_BLOCK, MF_MAX_NODES, MF_SLOTS, MF_MAX_GRID = 256, 42, 384, 1024      # csrc/pgo_internal.hpp
MIN_LM_DIAGONAL, MAX_LM_DIAGONAL = 1e-6, 1e32                          # pgo_options defaults (= Ceres)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# the operator
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
class Reference:
    """A [6 N x 6 N] csr (every keyframe as if free), b [6 N] the reduced negative gradient, diag [N, 6, 6] / grad [N, 6] the UNDAMPED sum J^T J blocks and J^T r before the
    switch elimination (what K2 writes), pair_off {(a, b): sum over the edges between a and b of J_a^T J_b} before the elimination, referenced [N]"""

    def __init__(self, A, b, diag, grad, pair_off, referenced, lam):
        self.A, self.b, self.diag, self.grad, self.pair_off, self.referenced, self.lam = A, b, diag, grad, pair_off, referenced, lam
        self.N = len(referenced)


def reference(O, G, q, t, s, radius, variant=None):
    """G: a graph of tests/normal_operator_cases.py (rel_c1 / rel_c2, sw_c1 / sw_c2 with switch e on switchable edge e, reg_node); O: the checker's problem of the same graph.
    variant: one deliberately wrong form —
      ("drop_side", e, side)        relative-pose edge e contributes nothing to the rows of its keyframe on `side`
      ("swap_parallel", e1, e2)     two edges on one pair exchange the Jacobian of their second keyframe in the coupling block J1^T J2
      ("omit_switch", e)            switchable edge e's rank-one elimination term is left out
      ("no_damping", n)             keyframe n gets no LM damping
      ("transpose", e)              relative-pose edge e's coupling block goes in transposed"""
    v = variant or ("none",)
    N = len(np.asarray(q).reshape(-1, 4))
    _, res, _ = O.evaluate(q, t, s)
    Er, Es, Ep = len(G.rel_c1), len(G.sw_c1), len(G.reg_node)
    r_rel, r_sw, r_pri = res[:6 * Er].reshape(Er, 6), res[6 * Er:6 * Er + 7 * Es].reshape(Es, 7), res[6 * Er + 7 * Es:].reshape(Ep, 6)
    diag, grad = np.zeros((N, 6, 6)), np.zeros((N, 6))
    referenced = np.zeros(N, bool)
    rows, cols, blocks = [], [], []      # off-diagonal 6 x 6 blocks, duplicates summed
    pair_off = {}

    def off(a, b, B):
        rows.append(a); cols.append(b); blocks.append(B)

    # relative-pose edges
    J1, J2, _ = O.jacobian_blocks(q, t, s, 0)
    for e in range(Er):
        a, b = int(G.rel_c1[e]), int(G.rel_c2[e])
        referenced[a] = referenced[b] = True
        Ja, Jb = J1[e], J2[e]
        Jb_c = Jb
        if v[0] == "swap_parallel" and e in v[1:]:
            Jb_c = J2[v[2] if e == v[1] else v[1]]
        B = Ja.T @ Jb_c
        pair_off[(a, b)] = pair_off.get((a, b), 0.0) + Ja.T @ Jb
        if v[0] == "transpose" and e == v[1]:
            B = B.T
        keep_a = not (v[0] == "drop_side" and e == v[1] and v[2] == 0)
        keep_b = not (v[0] == "drop_side" and e == v[1] and v[2] == 1)
        if keep_a:
            diag[a] += Ja.T @ Ja; off(a, b, B)
        if keep_b:
            diag[b] += Jb.T @ Jb; off(b, a, B.T)
        grad[a] += Ja.T @ r_rel[e]; grad[b] += Jb.T @ r_rel[e]
    # regularisers
    Jp, _, _ = O.jacobian_blocks(q, t, s, 2)
    for k in range(Ep):
        n = int(G.reg_node[k])
        referenced[n] = True
        diag[n] += Jp[k].T @ Jp[k]; grad[n] += Jp[k].T @ r_pri[k]
    # switchable edges: 7 residuals, the pose Jacobians fill the first 6 rows, dr/ds all 7
    K1, K2, ds = O.jacobian_blocks(q, t, s, 1)
    hss, gs = np.zeros(Es), np.zeros(Es)
    cc = np.zeros((Es, 2, 6))
    for e in range(Es):
        a, b = int(G.sw_c1[e]), int(G.sw_c2[e])
        referenced[a] = referenced[b] = True
        Ja, Jb = K1[e], K2[e]
        diag[a] += Ja.T @ Ja; diag[b] += Jb.T @ Jb
        pair_off[(a, b)] = pair_off.get((a, b), 0.0) + Ja.T @ Jb
        off(a, b, Ja.T @ Jb); off(b, a, Jb.T @ Ja)
        grad[a] += Ja.T @ r_sw[e, :6]; grad[b] += Jb.T @ r_sw[e, :6]
        cc[e, 0], cc[e, 1] = Ja.T @ ds[e, :6], Jb.T @ ds[e, :6]
        hss[e], gs[e] = ds[e] @ ds[e], ds[e] @ r_sw[e]
    undamped_diag, undamped_grad = diag.copy(), grad.copy()

    # the LM diagonal from the UNDAMPED diagonal of H, poses and switches alike
    def lm(d):
        scale = 1.0 / (1.0 + np.sqrt(d))
        return np.clip(scale ** 2 * d, MIN_LM_DIAGONAL, MAX_LM_DIAGONAL) / radius / scale ** 2
    lam = lm(np.einsum("nii->ni", diag).copy())
    if v[0] == "no_damping":
        lam[v[1]] = 0.0
    lam_s = lm(hss)
    # eliminate every switch by its own edge
    D = diag.copy()
    bvec = -grad
    for e in range(Es):
        if v[0] == "omit_switch" and e == v[1]:
            continue
        a, b = int(G.sw_c1[e]), int(G.sw_c2[e])
        ai = 1.0 / (hss[e] + lam_s[e])
        D[a] -= np.outer(cc[e, 0], cc[e, 0]) * ai; D[b] -= np.outer(cc[e, 1], cc[e, 1]) * ai
        off(a, b, -np.outer(cc[e, 0], cc[e, 1]) * ai); off(b, a, -np.outer(cc[e, 1], cc[e, 0]) * ai)
        bvec[a] += cc[e, 0] * gs[e] * ai; bvec[b] += cc[e, 1] * gs[e] * ai
    for n in range(N):
        D[n][np.arange(6), np.arange(6)] += lam[n]
    rows = np.concatenate([np.arange(N), np.asarray(rows, np.int64)]) if rows else np.arange(N)
    cols = np.concatenate([np.arange(N), np.asarray(cols, np.int64)]) if cols else np.arange(N)
    data = np.concatenate([D, np.asarray(blocks).reshape(-1, 6, 6)]) if blocks else D
    A = _block_coo(rows, cols, data, N)
    return Reference(A, bvec.reshape(-1), undamped_diag, undamped_grad, pair_off, referenced, lam)


def _block_coo(rows, cols, data, N):
    r = (rows[:, None, None] * 6 + np.arange(6)[None, :, None]) + np.zeros((1, 1, 6), np.int64)
    c = (cols[:, None, None] * 6 + np.arange(6)[None, None, :]) + np.zeros((1, 6, 1), np.int64)
    A = sp.coo_matrix((data.reshape(-1), (r.reshape(-1), c.reshape(-1))), shape=(6 * N, 6 * N)).tocsr()
    A.sum_duplicates()
    return A


def device_rows(ref, constant=()):
    """(A_dev csr, b_dev, free): the operator BOTH matvec forms of the device define (build_rows_kernel writes it for the assembled form and, as the damping plane with
    identity rows, for the matrix-free one; mf_spmv_kernel and apply_operator_kernel apply it):
      * a keyframe outside the system — constant, or referenced by no residual block — has the identity row: 1.0 on its diagonal, 0.0 elsewhere, b = 0;
      * its COLUMN is left as it is: the rows of its free neighbours keep their coupling block with it (neither matvec masks its input; every PCG vector is zero there,
        so the solver never multiplies that block by anything else); an unreferenced keyframe has no neighbour, its column is the unit vector too;
      * the diagonal blocks of free keyframes keep the J^T J terms (and the switch terms) of their edges to constant keyframes."""
    free = ref.referenced.copy()
    free[np.asarray(list(constant), dtype=np.int64)] = False
    keep = np.repeat(free, 6).astype(np.float64)
    A = sp.diags(keep) @ ref.A + sp.diags(1.0 - keep)
    return A.tocsr(), ref.b * keep, free


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# the comparison
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def block_maxima(M):
    """[N, N]: max-norm of every 6 x 6 block of a dense matrix"""
    n = M.shape[0] // 6
    return np.abs(M.reshape(n, 6, n, 6)).max(axis=(1, 3))


def compare(A_dev, A_ref):
    """dense operators -> dict(err: |A_dev - A_ref|max / |A_ref|max;  err_block: max over the 6 x 6 blocks (i, j) of |D_ij|max / max(|A_ii|max, |A_jj|max) — for a positive
    definite matrix |A_ij| <= sqrt(|A_ii| |A_jj|), so this is the scale at which block (i, j) matters: a wrong low-weight edge next to a hub cannot hide under the hub's norm;
    worst: the larger of the two;  nonzero_outside: entries of A_dev that are not exactly 0.0 in blocks where A_ref stores nothing)"""
    Dm = block_maxima(A_dev - A_ref)
    Rm = block_maxima(A_ref)
    d = np.diag(Rm)
    scale = np.maximum(d[:, None], d[None, :])
    err = float(Dm.max() / Rm.max())
    err_block = float((Dm / scale).max())
    outside = int(np.count_nonzero(block_maxima(A_dev)[Rm == 0.0]))
    return dict(err=err, err_block=err_block, worst=max(err, err_block), nonzero_outside=outside)


def row_block_scale(A, X):
    """[n_vec, N]: for y = A x the scale of keyframe i's six rows under the same block scaling: sum over the blocks (i, j) of row i of max(|A_ii|max, |A_jj|max) |x_j|max"""
    N = A.shape[0] // 6
    B = A.tocoo()
    P = sp.coo_matrix((np.ones(B.nnz), (B.row // 6, B.col // 6)), shape=(N, N)).tocsr().tocoo()      # the block pattern
    d = np.abs(diagonal_blocks(A)).max(axis=(1, 2))
    w = np.maximum(d[P.row], d[P.col])
    X = np.atleast_2d(X)
    out = np.zeros((len(X), N))
    for v in range(len(X)):
        xm = np.abs(X[v].reshape(N, 6)).max(axis=1)
        out[v] = np.bincount(P.row, weights=w * xm[P.col], minlength=N)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# the tile-closing rule
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def matrix_free_eligible(N, rel_c1, rel_c2, sw_c1, sw_c2, reg_node):
    deg = np.bincount(np.concatenate([rel_c1, rel_c2, sw_c1, sw_c2]).astype(np.int64), minlength=N)
    npri = np.bincount(np.asarray(reg_node, np.int64), minlength=N)
    return bool(deg.max(initial=0) <= MF_BLOCK and npri.max(initial=0) <= 1)


def tile_rule(N, rel_c1, rel_c2, sw_c1, sw_c2):
    """pack_mf_tiles' closing rule: whole keyframes in ascending order; a keyframe opens a new tile when with it the tile would hold more than MF_SLOTS edge sides or more
    than MF_BLOCK lanes (a relative-pose edge with both keyframes in the tile takes ONE lane for its two sides), or when the tile already holds MF_MAX_NODES keyframes.
    -> dict(node0 [tiles + 1], sides, lanes, pair_lanes [tiles], closed_by [tiles]: 'slots' / 'lanes' / 'nodes' / 'end')"""
    rel_c1, rel_c2 = np.asarray(rel_c1, np.int64), np.asarray(rel_c2, np.int64)
    deg = np.bincount(np.concatenate([rel_c1, rel_c2, np.asarray(sw_c1, np.int64), np.asarray(sw_c2, np.int64)]), minlength=N)
    lower = [[] for _ in range(N)]      # per keyframe: the other keyframe of each relative-pose edge to a LOWER keyframe
    for a, b in zip(rel_c1, rel_c2):
        if a != b:
            lower[max(a, b)].append(min(a, b))
    node0, sides_t, lanes_t, pairs_t, why = [0], [], [], [], []
    sides = pairs = cur = 0
    start = 0
    for n in range(N):
        d = int(deg[n])
        np_ = sum(1 for o in lower[n] if o >= start)
        reason = "slots" if sides + d > MF_SLOTS else "lanes" if sides + d - (pairs + np_) > MF_BLOCK else "nodes" if cur >= MF_MAX_NODES else None
        if reason:
            node0.append(n); sides_t.append(sides); lanes_t.append(sides - pairs); pairs_t.append(pairs); why.append(reason)
            sides = pairs = cur = 0
            start, np_ = n, 0
        sides += d; pairs += np_; cur += 1
    node0.append(N); sides_t.append(sides); lanes_t.append(sides - pairs); pairs_t.append(pairs); why.append("end")
    return dict(node0=np.array(node0), sides=np.array(sides_t), lanes=np.array(lanes_t), pair_lanes=np.array(pairs_t), closed_by=why, n_tiles=len(why))


def tile_invariants(T, N):
    """what any packing must keep (asserted on the Python rule's tables on the CPU and on the device's own on the GPU)"""
    node0 = np.asarray(T["node0"])
    assert node0[0] == 0 and node0[-1] == N and np.all(np.diff(node0) >= 1), "the tiles do not partition 0..N"
    assert np.diff(node0).max() <= MF_MAX_NODES and np.max(T["sides"]) <= MF_SLOTS and np.max(T["lanes"]) <= MF_BLOCK
    assert np.all(np.asarray(T["lanes"]) + np.asarray(T["pair_lanes"]) == np.asarray(T["sides"]))      # a pair lane serves two sides, every other lane one


def tile_condition(T, condition):
    """does a tile table meet a case's target condition?  'lanes256': a tile with 256 lanes; 'empty': a tile without lanes; 'lanes250': a tile of fewer than 42 keyframes with
    at least 250 lanes; 'pairs2': a tile with pair lanes (second slot) and other lanes; 'single': a last tile of one keyframe; None: no condition"""
    nn, lanes, pairs = np.diff(np.asarray(T["node0"])), np.asarray(T["lanes"]), np.asarray(T["pair_lanes"])
    if condition is None:
        return True
    if condition == "lanes256":
        return bool(np.any(lanes == MF_BLOCK))
    if condition == "empty":
        return bool(np.any(lanes == 0))
    if condition == "lanes250":
        return bool(np.any((nn < MF_MAX_NODES) & (lanes >= 250)))
    if condition == "pairs2":
        return bool(np.any((pairs >= 20) & (lanes - pairs >= 100)))
    if condition == "single":
        return bool(nn[-1] == 1 and len(nn) >= 2)
    raise ValueError(condition)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# textbook PCG with exact block inverses (sparse)
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def diagonal_blocks(A):
    N = A.shape[0] // 6
    D = np.zeros((N, 6, 6))
    A = A.tocsr()
    for k in range(6):
        for l in range(6):
            D[:, k, l] = np.asarray(A[k::6, l::6].diagonal()).reshape(-1)
    return D


def block_jacobi_factors(D, fp32=False):
    """[N, 6, 6] D^-1 of every block: exact, or (fp32) through the packed Cholesky factor the device keeps, as tests/precond_model.py::block_jacobi rounds it"""
    if not fp32:
        return np.linalg.inv(D)
    L = np.linalg.cholesky(D)
    f32 = lambda M: M.astype(np.float32).astype(np.float64)
    idx = np.arange(6)
    Lr = f32(np.tril(L, -1))
    Lr[:, idx, idx] = 1.0 / f32(1.0 / L[:, idx, idx])
    Li = np.linalg.inv(Lr)
    return np.einsum("nki,nkj->nij", Li, Li)


def pcg(A, b, Dinv, k):
    """k steps of textbook block-Jacobi PCG from x = 0 (as tests/precond_model.py::pcg); returns [x_1 .. x_k]"""
    apply = lambda r: np.einsum("nij,nj->ni", Dinv, r.reshape(-1, 6)).reshape(-1)
    x = np.zeros_like(b)
    r = b.copy()
    z = apply(r)
    p = z.copy()
    rz = r @ z
    out = []
    for _ in range(k):
        qv = A @ p
        alpha = rz / (p @ qv)
        x = x + alpha * p
        r = r - alpha * qv
        z = apply(r)
        rz_new = r @ z
        p = z + (rz_new / rz) * p
        rz = rz_new
        out.append(x.copy())
    return out
