"""A plain dense fp64 model (numpy only) of the three preconditioners and of the PCG around them: what the HIP kernels are compared with in
tests/test_gpu_precond_operator.py, itself checked on the CPU in tests/test_precond_model.py.

Everything is a dense matrix over the FREE keyframes (6 rows each, global keyframe order; constant and unreferenced keyframes are deleted):

  system      A = damped Schur complement of the checker's dense H at a trust-region radius, b = reduced negative gradient (as
              tests/test_gpu_parity.py::test_normal_operator_is_schur_complement builds A)
  block-Jacobi   D^-1 = inverses of the 6x6 diagonal blocks of A
  two-level   M^-1 = D^-1 + P (P^T A P)^-1 P^T, aggregates = runs of m consecutive keyframes (m by the rule of build_two_level_aggregates), centroids over
              the free members, P_i = [[I, 0], [-2 [d_i]x, I]]; an aggregate without a free keyframe contributes nothing; m = 1 (one aggregate per keyframe):
              the coarse term REPLACES D^-1 (coarse_prolong_kernel: z = Ac^-1 r), M^-1 = A^-1
  multigrid   M^-1 = D^-1 + s P_0 V(P_0^T r), V = the V(1,1) cycle of csrc/pgo_mg_kernels.hpp's header comment over Galerkin levels, damped block-Jacobi
              (omega) on every sparse level, every coarse correction scaled by s (launch_mg_apply), the top level inverted densely; a smoothed transition:
              Ps = (I - c Dinv A) P with c = omega_p / omega, Dinv = omega D^-1, level above = Ps^T A Ps, applied implicitly or through the
              explicit transfer operator R^T = Ps - Dinv A Ps; the smoother's safety rescaling: a level whose estimate omega * lambda (power_estimate) exceeds 1.75 gets
              its Dinv scaled to omega * lambda = 1.5 before anything above it is formed; the smoothed keyframe transition (smoothed_fine): Ps_0 = (I - omega_p D^-1 A) P_0,
              level 1 = Ps_0^T A Ps_0, M^-1 = D^-1 + s Ps_0 V Ps_0^T

fp32 mode: every object the device streams in fp32 — the level matrices inside the cycle, R^T, Ps_0, the dense inverse, the two-level Ac^-1, the packed block-Jacobi
Cholesky factors — is rounded with astype(np.float32) and accumulated in fp64.  `variant` switches in the deliberately wrong forms the CPU tests use to show that
the GPU test's tolerance would catch them."""
import numpy as np

OMEGA, OMEGA_P, SMOOTHER_LIMIT, SMOOTHER_TARGET = 0.9, 0.6, 1.75, 1.5      # pgo_options defaults; mg_rescale_dinv_kernel's limit and target


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# the system
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
class Linearisation:
    """the checker's dense H and gradient at one state: everything the system needs at any radius"""

    def __init__(self, O, g, q, t, s, constant=()):
        self.N, self.S = g.n_poses, len(s)
        self.H = O.dense_normal_matrix(q, t, s)
        _, _, self.grad = O.evaluate(q, t, s)
        self.t = np.asarray(t, dtype=np.float64).reshape(-1, 3).copy()
        ref = np.zeros(self.N, bool)
        for c in (g.odom_c1, g.odom_c2, g.loop_c1, g.loop_c2, g.reg_node):
            ref[np.asarray(c, dtype=np.int64)] = True
        free = ref.copy()
        free[np.asarray(list(constant), dtype=np.int64)] = False
        self.free = free                                                   # [N] part of the system
        self.idx = np.flatnonzero(free)                                    # free keyframes, ascending
        self.rows = (self.idx[:, None] * 6 + np.arange(6)).reshape(-1)     # their rows among all 6 N

    def system(self, radius):
        """(A, b) over the free keyframes: damped Schur complement, reduced negative gradient"""
        H, N = self.H, self.N
        d = np.diag(H)
        scale = 1.0 / (1.0 + np.sqrt(d))
        lam = np.clip(scale ** 2 * d, 1e-6, 1e32) / radius / scale ** 2
        Hd = H + np.diag(lam)
        n6 = 6 * N
        if Hd.shape[0] > n6:
            X = np.linalg.solve(Hd[n6:, n6:], np.column_stack([Hd[n6:, :n6], self.grad[n6:]]))
            A = Hd[:n6, :n6] - Hd[:n6, n6:] @ X[:, :n6]
            b = -(self.grad[:n6] - Hd[:n6, n6:] @ X[:, n6])
        else:
            A, b = Hd, -self.grad[:n6]
        A = A[np.ix_(self.rows, self.rows)]
        return 0.5 * (A + A.T), b[self.rows].copy()

    def expand(self, M):
        """a matrix over the free keyframes -> over all 6 N rows (zero rows and columns outside the system)"""
        out = np.zeros((6 * self.N, 6 * self.N))
        out[np.ix_(self.rows, self.rows)] = M
        return out

    def expand_vec(self, x):
        out = np.zeros(6 * self.N)
        out[self.rows] = x
        return out


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# pieces
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def f32(M):
    return M.astype(np.float32).astype(np.float64)


def diag_blocks(A):
    n = A.shape[0] // 6
    return np.stack([A[6 * i:6 * i + 6, 6 * i:6 * i + 6] for i in range(n)])


def block_diag(blocks):
    n = len(blocks)
    M = np.zeros((6 * n, 6 * n))
    for i in range(n):
        M[6 * i:6 * i + 6, 6 * i:6 * i + 6] = blocks[i]
    return M


def block_jacobi(A, fp32=False):
    """D^-1 as a dense matrix.  fp32: through the packed Cholesky factor the device keeps (invert_rows_kernel: off-diagonal entries of L and 1 / L_ii rounded to fp32)"""
    D = diag_blocks(A)
    if not fp32:
        return block_diag(np.linalg.inv(D))
    out = []
    for Di in D:
        L = np.linalg.cholesky(Di)
        Lr = f32(np.tril(L, -1)) + np.diag(1.0 / f32(1.0 / np.diag(L)))
        Li = np.linalg.inv(Lr)
        out.append(Li.T @ Li)
    return block_diag(np.stack(out))


def skew(d):
    return np.array([[0.0, -d[2], d[1]], [d[2], 0.0, -d[0]], [-d[1], d[0], 0.0]])


def rigid_block(d, factor=2.0, cross=True):
    """B_i: dtheta_i = y_theta, dt_i = y_t - 2 d_i x y_theta"""
    B = np.eye(6)
    if cross:
        B[3:, :3] = -factor * skew(d)
    return B


def prolongation(d, agg, n_coarse, factor=2.0, cross=True):
    """P [6 n x 6 n_coarse]: block row i, block column agg[i] = B_i(d_i)"""
    n = len(agg)
    P = np.zeros((6 * n, 6 * n_coarse))
    for i in range(n):
        P[6 * i:6 * i + 6, 6 * agg[i]:6 * agg[i] + 6] = rigid_block(d[i], factor, cross)
    return P


def two_level_aggregates(N, coarse_aggregates):
    """(m, n_agg) by the rule of build_two_level_aggregates (csrc/pgo_pcg.hip); None: the graph gets no two-level method"""
    n_agg = coarse_aggregates
    half = min(n_agg // 2, 256)
    n_agg = N if N <= half else min(n_agg, max(N // 8, half))
    if n_agg < 2 or (N + n_agg - 1) // n_agg > 1024:
        return None
    m = (N + n_agg - 1) // n_agg
    return m, (N + m - 1) // m


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# two-level method
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def two_level(lin, A, m, fp32=False, variant=None):
    """-> dict(M, C, P, Ac_inv): M^-1, its coarse correction C = P Ac^-1 P^T, both dense over the free keyframes"""
    v = variant or {}
    idx, t = lin.idx, lin.t
    agg_all = np.arange(lin.N) // m
    present = np.unique(agg_all[idx])                          # aggregates with a free keyframe; the others contribute nothing
    renum = -np.ones(agg_all.max() + 1, np.int64)
    renum[present] = np.arange(len(present))
    agg = renum[agg_all[idx]]
    cen = np.zeros((len(present), 3))
    for a, ga in enumerate(present):
        members = np.flatnonzero(agg_all == ga) if v.get("centroid_all") else idx[agg_all[idx] == ga]
        cen[a] = t[members].mean(axis=0)
    d = t[idx] - cen[agg]
    P = prolongation(d, agg, len(present), factor=v.get("factor", 2.0))
    R = prolongation(d, agg, len(present), factor=v.get("factor", 2.0), cross=not v.get("restrict_no_cross")).T
    Ac = P.T @ A @ P
    if v.get("transfer_centroid_all"):                         # Ac from the free members' centroids, restriction and prolongation with the centroids over all members
        cen2 = np.stack([t[np.flatnonzero(agg_all == ga)].mean(axis=0) for ga in present])
        P = prolongation(t[idx] - cen2[agg], agg, len(present))
        R = P.T
    Ac_inv = np.linalg.inv(0.5 * (Ac + Ac.T))
    Ac_inv = 0.5 * (Ac_inv + Ac_inv.T)
    if fp32:
        Ac_inv = f32(Ac_inv)
    C = P @ Ac_inv @ R
    M = C if m == 1 else block_jacobi(A, fp32) + C
    return dict(M=M, C=C, P=P, Ac_inv=Ac_inv, agg=agg, d=d)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# multigrid
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def power_estimate(Dinv_unit, A, steps=8):
    """launch_mg_level_power: lambda_max(D^-1 A) from eight un-normalised power steps on the fixed start vector"""
    n6 = A.shape[0]
    v = 1.0 + 0.5 * np.sin(0.7 * np.arange(n6))
    w = v
    for _ in range(steps):
        w, v = v, Dinv_unit @ (A @ v)
    return np.sqrt((v @ v) / (w @ w))


def multigrid(lin, A, agg0, parents, fp32=False, omega=OMEGA, scale=1.0, omega_p=OMEGA_P, smoothed_levels=0, explicit=False, smoothed_fine=False, variant=None):
    """agg0 [N]: level-1 node of every keyframe (-1 outside the system); parents[l - 1] (l = 1 .. n_levels - 1): level-(l+1) node of every level-l node.
    smoothed_fine: the transition keyframes -> level 1 is smoothed as well (launch_mg_assemble_fine): Ps_0 = P_0 - c (omega D^-1) A P_0 with D the diagonal
    blocks of A itself (mg_dinv_kernel on the keyframe level: fp64, no power estimate, no rescaling), level 1 = Ps_0^T (A Ps_0), M^-1 = D^-1 + s Ps_0 V Ps_0^T; the cycle
    streams Ps_0 as fp32 blocks, the same rounded numbers in both orientations (mg_ps_f32_kernel).
    -> dict(M, C = M - D^-1, V [the cycle as a matrix on level 1], A1 [level 1], levels, lam_max [exact lambda_max(D^-1 A) per sparse level], lam_est [the device's
    estimate of it], rescaled [per sparse level: that estimate exceeds the limit], limit_active [any of them])
    variant: the wrong devices of tests/test_precond_model.py.  Rescaling: no_rescale (the limit is never applied), rescale_every_level (the factor of the first level that
    triggers on all sparse levels), ps_before_rescale (Ps, W and R^T of a smoothed transition from the unrescaled Dinv, the cycle with the rescaled one).  Smoothed keyframe
    transition: fine_restrict_plain (restriction with P_0^T), fine_level1_plain (level 1 = P_0^T A P_0), fine_omega_p (omega in omega_p's place in Ps_0)."""
    v = variant or {}
    if v.get("rescale_every_level") and "_factor_all" not in v:
        base = multigrid(lin, A, agg0, parents, fp32, omega, scale, omega_p, smoothed_levels, explicit, smoothed_fine, {k: x for k, x in v.items() if k != "rescale_every_level"})
        first = [omega * e for e, on in zip(base["lam_est"], base["rescaled"]) if on]
        v = dict(v, _factor_all=SMOOTHER_TARGET / first[0] if first else 1.0)
    factor = v.get("factor", 2.0)
    idx, t = lin.idx, lin.t
    a0 = np.asarray(agg0)[idx]
    assert np.all(a0 >= 0) and np.all(np.asarray(agg0)[~lin.free] < 0), "the hierarchy's keyframes are not the system's"
    n1 = int(a0.max()) + 1
    pos = np.stack([t[idx[a0 == a]].mean(axis=0) for a in range(n1)])
    P0 = prolongation(t[idx] - pos[a0], a0, n1, factor=factor)
    R0 = prolongation(t[idx] - pos[a0], a0, n1, factor=factor, cross=not v.get("restrict_no_cross")).T
    levels = []
    cs = omega_p / omega
    T0 = P0                                                  # what the cycle prolongs to the keyframes with; R0: what it restricts with
    if smoothed_fine:
        Dinv0 = omega * block_diag(np.linalg.inv(diag_blocks(A)))
        Ps0 = P0 - (1.0 if v.get("fine_omega_p") else cs) * Dinv0 @ (A @ P0)
        Al = P0.T @ A @ P0 if v.get("fine_level1_plain") else Ps0.T @ (A @ Ps0)
        T0 = f32(Ps0) if fp32 else Ps0
        R0 = P0.T if v.get("fine_restrict_plain") else T0.T
    else:
        Al = P0.T @ A @ P0
    A1 = 0.5 * (Al + Al.T)
    lam_max, lam_est, rescaled = [], [], []
    for li, par in enumerate(parents):                       # sparse level li + 1
        par = np.asarray(par)
        n_next = int(par.max()) + 1
        pos_next = np.stack([pos[par == a].mean(axis=0) for a in range(n_next)])
        P = prolongation(pos - pos_next[par], par, n_next, factor=factor)
        Al = 0.5 * (Al + Al.T)
        Dunit = block_diag(np.linalg.inv(diag_blocks(Al)))
        Af = f32(Al) if fp32 else Al
        Dh = block_diag(np.linalg.inv(np.linalg.cholesky(diag_blocks(Al))))      # L^-1 per block: L^-1 A L^-T is similar to D^-1 A
        lam_max.append(float(np.linalg.eigvalsh(Dh @ Al @ Dh.T)[-1]))
        est = power_estimate(Dunit, Af)
        lam_est.append(float(est))
        Dinv = Dplain = omega * Dunit
        rescaled.append(bool(omega * est > SMOOTHER_LIMIT))
        if "_factor_all" in v:
            Dinv = Dinv * v["_factor_all"]
        elif rescaled[-1] and not v.get("no_rescale"):
            Dinv = Dinv * (SMOOTHER_TARGET / (omega * est))
        L = dict(A=Al, Af=Af, Dinv=Dinv, P=P, smoothed=li < smoothed_levels, explicit=explicit)
        if L["smoothed"]:
            Dps = Dplain if v.get("ps_before_rescale") else Dinv
            Ps = P - cs * Dps @ (Al @ P)
            W = Al @ Ps
            RT = Ps - Dps @ W
            L.update(Ps=Ps, RTf=f32(RT) if fp32 else RT)
            A_next = Ps.T @ W
        else:
            A_next = P.T @ Al @ P
        levels.append(L)
        Al, pos = A_next, pos_next
    Al = 0.5 * (Al + Al.T)
    top_inv = np.linalg.inv(Al)
    top_inv = 0.5 * (top_inv + top_inv.T)
    if fp32:
        top_inv = f32(top_inv)
    drop_post = v.get("drop_post_level", -1)                 # 1-based sparse level whose post-smoothing step is dropped

    def cycle(l, r):                                         # l: 0-based index into levels; len(levels): the dense level
        if l == len(levels):
            return top_inv @ r
        L = levels[l]
        Af, Dinv, P = L["Af"], L["Dinv"], L["P"]
        post = 0.0 if drop_post == l + 1 else 1.0
        x = Dinv @ r
        if L["smoothed"] and L["explicit"]:
            vv = x + Dinv @ (r - Af @ x)
            xn = cycle(l + 1, L["RTf"].T @ r)
            return vv + scale * (L["RTf"] @ xn)
        if L["smoothed"]:
            tt = r - Af @ x
            u = cs * (Dinv @ tt)
            xn = cycle(l + 1, P.T @ (tt - Af @ u))
            e = scale * (P @ xn)
            y = x + e - cs * (Dinv @ (Af @ e))
        else:
            xn = cycle(l + 1, P.T @ (r - Af @ x))
            y = x + scale * (P @ xn)
        return y + post * (Dinv @ (r - Af @ y))

    V = cycle(0, np.eye(6 * n1))                             # the cycle is linear: applied to the identity of level 1
    C = scale * (T0 @ V @ R0)
    M = block_jacobi(A, fp32) + C
    return dict(M=M, C=C, V=V, A1=A1, levels=levels, lam_max=lam_max, lam_est=lam_est, rescaled=rescaled, limit_active=any(rescaled), n_levels=len(levels) + 1)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# reference PCG
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def pcg(A, b, Minv, k):
    """k steps of textbook preconditioned CG from x = 0 (Minv: dense matrix); returns [x_1 .. x_k]"""
    x = np.zeros_like(b)
    r = b.copy()
    z = Minv @ r
    p = z.copy()
    rz = r @ z
    out = []
    for _ in range(k):
        q = A @ p
        alpha = rz / (p @ q)
        x = x + alpha * p
        r = r - alpha * q
        z = Minv @ r
        rz_new = r @ z
        p = z + (rz_new / rz) * p
        rz = rz_new
        out.append(x.copy())
    return out


def pcg_iterations(A, b, Minv, tol, max_iterations=5000):
    """iterations textbook PCG needs until r.z <= tol^2 r0.z0"""
    x = np.zeros_like(b)
    r = b.copy()
    z = Minv @ r
    p = z.copy()
    rz = rz0 = r @ z
    for k in range(1, max_iterations + 1):
        q = A @ p
        alpha = rz / (p @ q)
        x += alpha * p
        r -= alpha * q
        z = Minv @ r
        rz_new = r @ z
        if rz_new <= tol * tol * rz0:
            return k
        p = z + (rz_new / rz) * p
        rz = rz_new
    return max_iterations


def maxnorm(M):
    return float(np.abs(M).max())
