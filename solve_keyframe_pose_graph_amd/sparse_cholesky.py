"""ctypes binding of libpgo_sparse.so (include/pgo_sparse.h): the tile-sparse exact Cholesky solver on the GPU, for systems above capi.DENSE_MAX_KEYFRAMES, and
covariance blocks from it.

The library is a companion of libpgo.so: it takes no Problem.  covariance() below carries a Problem's system across with Problem.normal_blocks() — every handle has
them, matrix-free ones too — and returns what Problem.covariance returns where that runs; covariance_all() returns every keyframe's marginal and every edge's joint
covariance from one selected inverse of the factor (SparseCholesky.selected_inverse / selected_blocks); cross_covariance() returns the blocks of ANY keyframe pairs, in
any number — those of keyframes that share no edge yet, outside the factor's pattern — from SparseCholesky.inverse_columns, and loop_candidate_gate() the chi-square gate
of loop-closure candidates built on them.  Graph is a pose graph that linearises itself in this library (yaw/pitch/roll-weighted edges included), solve_graph() the
exact solve on it without a Problem; YawGraph and solve_yaw_graph() are the same for the reference's 4-DoF (yaw + translation) formulation.  solve_exact() is Problem.solve with every LM step exact, at any keyframe count: the Problem linearises and steps on the manifold
through its hooks (as callbacks), SparseLm solves every damped system on the factor's tiles, the decisions are csrc/pgo_lm.hpp's.  As capi: no CPU fallback, a missing
library or device is an error."""
import ctypes as C
import dataclasses

import numpy as np

from . import _build
from .capi import PgoError

ORDER_AUTO, ORDER_NATURAL, ORDER_RCM = -1, 0, 1      # PGO_SPARSE_ORDER_*
MAX_RHS, MAX_GROUPS = 65535, 64                      # PGO_SPARSE_MAX_RHS, PGO_SPARSE_MAX_GROUPS
ERR_INVALID_ARG, ERR_STATE, ERR_NUMERIC = -1, -5, -7
# what info() and spd_solve() report of a plan
INFO = ("nt", "a_tiles", "l_tiles", "ordering", "bytes", "factor_launches", "solve_launches", "tile_updates")
SELECTED_INFO = ("launches", "tile_products", "bytes", "current")      # selected_info()
COLUMNS_INFO = ("launches", "tile_products", "bytes", "chunks")        # columns_info()
WORKSPACE_BYTES = 1 << 30                                               # PGO_SPARSE_WORKSPACE_BYTES

_dp, _ip, _lp, _bp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_uint8)
_lib = None

# pgo_sparse_lm_callbacks: pgo_evaluate, pgo_get_normal_blocks and pgo_manifold_plus without the handle
EVALUATE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, _dp, _dp, _dp, C.c_int64, C.c_int64, _dp, _dp, _dp)
NORMAL_BLOCKS_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, _dp, _dp, _dp, _dp, _dp, _dp)
MANIFOLD_PLUS_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int64, _dp, _dp, _dp, _dp, _dp)
LM_TIMES = ("upload_ms", "fill_ms", "factor_ms", "solve_ms", "backsub_model_ms", "download_ms")      # pgo_sparse_lm_last_times


class LmCallbacks(C.Structure):
    _fields_ = [("evaluate", EVALUATE_FN), ("normal_blocks", NORMAL_BLOCKS_FN), ("manifold_plus", MANIFOLD_PLUS_FN)]


def load(build=True):
    global _lib
    if _lib is not None:
        return _lib
    path = _build.build_libpgo_sparse() if build else _build.LIBSPARSE
    lib = C.CDLL(path)
    for f in _build.SPARSE_EXPORTS:
        if not hasattr(lib, f):
            raise RuntimeError("libpgo_sparse.so does not export %s" % f)
    lib.pgo_sparse_strerror.restype = C.c_char_p
    lib.pgo_sparse_strerror.argtypes = [C.c_int]
    lib.pgo_sparse_last_error.restype = C.c_char_p
    lib.pgo_sparse_last_error.argtypes = [C.c_void_p]
    lib.pgo_sparse_chol_last_ms.restype = C.c_double
    lib.pgo_sparse_chol_last_ms.argtypes = [C.c_void_p]
    lib.pgo_sparse_chol_destroy.restype = None
    lib.pgo_sparse_chol_destroy.argtypes = [C.c_void_p]
    lib.pgo_sparse_spd_solve.argtypes = [C.c_int32, C.c_int32, _dp, _dp, _ip, _dp, _lp, C.c_int32, C.POINTER(C.c_double)]
    lib.pgo_sparse_chol_create.argtypes = [C.c_int32, C.c_int64, _bp, C.c_int64, _ip, _ip, C.c_int32, C.POINTER(C.c_void_p)]
    lib.pgo_sparse_chol_info.argtypes = [C.c_void_p, _lp, _ip]
    lib.pgo_sparse_chol_factor.argtypes = [C.c_void_p, _dp, _dp]
    lib.pgo_sparse_chol_solve.argtypes = [C.c_void_p, C.c_int64, _dp, _dp]
    lib.pgo_sparse_chol_inverse_blocks.argtypes = [C.c_void_p, C.c_int64, _lp, _lp, _ip, _dp, C.c_int64, _ip, _ip, _dp]
    lib.pgo_sparse_chol_selected_inverse.argtypes = [C.c_void_p]
    lib.pgo_sparse_chol_selected_info.argtypes = [C.c_void_p, _lp]
    lib.pgo_sparse_chol_selected_blocks.argtypes = [C.c_void_p, C.c_int64, _ip, _ip, _dp, _bp]
    lib.pgo_sparse_chol_inverse_columns.argtypes = [C.c_void_p, C.c_int64, _ip, C.c_int64, _ip, _ip, _dp]
    lib.pgo_sparse_chol_columns_info.argtypes = [C.c_void_p, _lp]
    lib.pgo_sparse_chol_set_workspace_limit.argtypes = [C.c_void_p, C.c_int64]
    lib.pgo_sparse_reduce_normal_blocks.argtypes = [C.c_int64, _bp, _dp, _dp, _dp, _dp, C.c_int64, _ip, _ip, C.c_int64, _ip, _ip, _lp, _ip, _ip, _dp, _dp]
    lib.pgo_sparse_lm_create.argtypes = [C.c_void_p, C.c_int64, _bp, C.c_int64, _ip, _ip, C.c_int64, _ip, _ip, C.POINTER(C.c_void_p)]
    lib.pgo_sparse_lm_destroy.restype = None
    lib.pgo_sparse_lm_destroy.argtypes = [C.c_void_p]
    lib.pgo_sparse_lm_set_scale.argtypes = [C.c_void_p, _dp, _dp]
    lib.pgo_sparse_lm_step.argtypes = [C.c_void_p] + [_dp] * 6 + [C.c_double] * 3 + [_dp] * 3
    lib.pgo_sparse_lm_last_times.argtypes = [C.c_void_p, _dp]
    lib.pgo_sparse_lm_solve.argtypes = [C.c_void_p, C.POINTER(LmCallbacks), C.c_void_p, C.c_int64, _ip, _dp, _dp, _dp, C.c_void_p, C.c_void_p]
    lib.pgo_sparse_graph_create.argtypes = [C.c_int64, C.c_int32, C.POINTER(C.c_void_p)]
    lib.pgo_sparse_graph_destroy.restype = None
    lib.pgo_sparse_graph_destroy.argtypes = [C.c_void_p]
    lib.pgo_sparse_graph_add_relpose_edges.argtypes = [C.c_void_p, C.c_int64, _ip, _ip, _dp, _dp, _dp, C.c_int32, C.c_double]
    lib.pgo_sparse_graph_add_switchable_edges.argtypes = [C.c_void_p, C.c_int64, _ip, _ip, _dp, _ip, _dp, C.c_int32, C.c_double]
    lib.pgo_sparse_graph_set_node_regularizers.argtypes = [C.c_void_p, C.c_int64, _ip, _dp, _dp]
    lib.pgo_sparse_graph_set_nodes_constant.argtypes = [C.c_void_p, C.c_int64, _ip]
    lib.pgo_sparse_graph_finalize.argtypes = [C.c_void_p]
    lib.pgo_sparse_graph_evaluate.argtypes = [C.c_void_p, _dp, _dp, _dp, C.c_int64, C.c_int64, _dp, _dp, _dp]
    lib.pgo_sparse_graph_normal_blocks.argtypes = [C.c_void_p] + [_dp] * 6
    lib.pgo_sparse_graph_jacobian_blocks.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, _dp, _dp, _dp]
    lib.pgo_sparse_graph_manifold_plus.argtypes = [C.c_void_p, C.c_int64, _dp, _dp, _dp, _dp, _dp]
    lib.pgo_sparse_graph_lm_callbacks.argtypes = [C.c_void_p, C.POINTER(LmCallbacks), C.POINTER(C.c_void_p)]
    lib.pgo_sparse_graph_edge_lists.argtypes = [C.c_void_p, _lp, _bp, _bp] + [_ip] * 7
    lib.pgo_sparse_graph_last_times.argtypes = [C.c_void_p, _dp]
    lib.pgo_sparse_yaw_graph_create.argtypes = [C.c_int64, C.c_int32, C.POINTER(C.c_void_p)]
    lib.pgo_sparse_yaw_graph_destroy.restype = None
    lib.pgo_sparse_yaw_graph_destroy.argtypes = [C.c_void_p]
    lib.pgo_sparse_yaw_graph_add_edges.argtypes = [C.c_void_p, C.c_int64, _ip, _ip, _dp, _dp, _dp, _dp, _dp]
    lib.pgo_sparse_yaw_graph_set_nodes_constant.argtypes = [C.c_void_p, C.c_int64, _ip]
    lib.pgo_sparse_yaw_graph_finalize.argtypes = [C.c_void_p]
    lib.pgo_sparse_yaw_graph_evaluate.argtypes = [C.c_void_p, _dp, _dp, C.c_int64, _dp, _dp, _dp]
    lib.pgo_sparse_yaw_graph_normal_blocks.argtypes = [C.c_void_p] + [_dp] * 3
    lib.pgo_sparse_yaw_graph_jacobian_blocks.argtypes = [C.c_void_p, C.c_int64, C.c_int64, _dp, _dp]
    lib.pgo_sparse_yaw_graph_manifold_plus.argtypes = [C.c_void_p, C.c_int64, _dp, _dp, _dp, _dp, _dp]
    lib.pgo_sparse_yaw_graph_lm_callbacks.argtypes = [C.c_void_p, C.POINTER(LmCallbacks), C.POINTER(C.c_void_p)]
    lib.pgo_sparse_yaw_graph_edge_lists.argtypes = [C.c_void_p, _lp, _bp, _bp] + [_ip] * 4
    lib.pgo_sparse_yaw_graph_last_times.argtypes = [C.c_void_p, _dp]
    _lib = lib
    return lib


def _d(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _p(a, t):
    return a.ctypes.data_as(t) if a is not None and a.size else None


def _check(rc, h=None):
    if rc != 0:
        lib = load()
        raise PgoError(rc, "%s — %s" % (lib.pgo_sparse_strerror(rc).decode(), lib.pgo_sparse_last_error(h).decode()))


def spd_solve(a, b, pos=None, launches=1, device_id=0):
    """the tile-sparse factor and sweep launches on a symmetric positive definite matrix, row i at position pos[i]; returns (solution, plan figures, average
    milliseconds).  In natural order the solution equals capi.Problem.dense_spd_solve's as numbers."""
    a, b = _d(a), _d(b)
    n = a.shape[0]
    assert a.shape == (n, n) and b.shape == (n,)
    p = None if pos is None else _i(pos)
    assert p is None or p.shape == (n,)
    x, info, ms = np.empty(n), np.zeros(8, np.int64), C.c_double(0)
    _check(load().pgo_sparse_spd_solve(device_id, n, _p(a, _dp), _p(b, _dp), None if p is None else p.ctypes.data_as(_ip), x.ctypes.data_as(_dp), info.ctypes.data_as(_lp), launches, C.byref(ms)))
    return x, dict(zip(INFO, [int(v) for v in info])), ms.value


def reduce_normal_blocks(n_nodes, node_free, diag, offdiag, sw_c, sw_hss, rel_c1, rel_c2, swe_c1, swe_c2):
    """host only: the undamped Schur complement of Problem.normal_blocks()' arrays as blocks -> (pair_hi, pair_lo, s_diag (n_nodes, 6, 6), s_blocks (n_pairs, 6, 6))"""
    free = np.ascontiguousarray(node_free, dtype=np.uint8)
    rc1, rc2, sc1, sc2 = _i(rel_c1), _i(rel_c2), _i(swe_c1), _i(swe_c2)
    diag, offdiag, sw_c, sw_hss = _d(diag), _d(offdiag), _d(sw_c), _d(sw_hss)
    E = len(rc1) + len(sc1)
    assert free.shape == (n_nodes,) and diag.size == 36 * n_nodes and offdiag.size == 36 * E and sw_c.size == 12 * len(sc1) and sw_hss.size == len(sc1) and len(rc2) == len(rc1) and len(sc2) == len(sc1)
    n = C.c_int64(0)
    hi, lo, sd, sb = np.zeros(E, np.int32), np.zeros(E, np.int32), np.zeros((n_nodes, 6, 6)), np.zeros((E, 6, 6))
    _check(load().pgo_sparse_reduce_normal_blocks(n_nodes, _p(free, _bp), _p(diag, _dp), _p(offdiag, _dp), _p(sw_c, _dp), _p(sw_hss, _dp), len(rc1), _p(rc1, _ip), _p(rc2, _ip),
                                                  len(sc1), _p(sc1, _ip), _p(sc2, _ip), C.byref(n), _p(hi, _ip), _p(lo, _ip), _p(sd, _dp), _p(sb, _dp)))
    return hi[:n.value].copy(), lo[:n.value].copy(), sd, sb[:n.value].copy()


class SparseCholesky:
    """pgo_sparse_chol: the symbolic phase at construction (the keyframes of the system and the pairs that share a block), then factor / solve / inverse_blocks,
    and selected_inverse / selected_blocks for many blocks at once"""

    def __init__(self, n_nodes, in_system, pair_hi, pair_lo, ordering=ORDER_AUTO, device_id=0):
        self.lib = load()
        self.h = C.c_void_p()
        self.n_nodes = int(n_nodes)
        ins = np.ascontiguousarray(in_system, dtype=np.uint8)
        hi, lo = _i(pair_hi), _i(pair_lo)
        assert ins.shape == (self.n_nodes,) and hi.shape == lo.shape
        self.n_pairs = len(hi)
        _check(self.lib.pgo_sparse_chol_create(device_id, self.n_nodes, _p(ins, _bp), self.n_pairs, _p(hi, _ip), _p(lo, _ip), ordering, C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.lib.pgo_sparse_chol_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        """(plan figures, order): order[q] = the keyframe at position q"""
        info, order = np.zeros(8, np.int64), np.zeros(self.n_nodes, np.int32)
        _check(self.lib.pgo_sparse_chol_info(self.h, info.ctypes.data_as(_lp), order.ctypes.data_as(_ip)), self.h)
        return dict(zip(INFO, [int(v) for v in info])), order

    def last_ms(self):
        """HIP-event milliseconds of the launches of the last factor, solve, inverse_blocks, selected_inverse, selected_blocks or inverse_columns"""
        return self.lib.pgo_sparse_chol_last_ms(self.h)

    def factor(self, diag, pair_blocks):
        diag, blocks = _d(diag), _d(pair_blocks)
        assert diag.size == 36 * self.n_nodes and blocks.size == 36 * self.n_pairs
        _check(self.lib.pgo_sparse_chol_factor(self.h, _p(diag, _dp), _p(blocks, _dp)), self.h)

    def solve(self, B):
        """A^-1 B for the rows of B (n_rhs x 6 n_nodes, or one vector), keyframes in the caller's order"""
        B = _d(B)
        rows = B.reshape(1, -1) if B.ndim == 1 else B
        assert rows.shape[1] == 6 * self.n_nodes
        X = np.empty_like(rows)
        _check(self.lib.pgo_sparse_chol_solve(self.h, rows.shape[0], rows.ctypes.data_as(_dp), X.ctypes.data_as(_dp)), self.h)
        return X.reshape(B.shape)

    def inverse_blocks(self, groups, pairs):
        """groups: a list of groups, each a list of 1 or 6 sparse rows (cols, vals) over the 6 n_nodes coordinates; pairs: [(group a, group b), ...].
        Returns the list of V_a A^-1 V_b^T, (d_a, d_b) arrays."""
        group_ptr, row_ptr, col, val = [0], [0], [], []
        for g in groups:
            for cols, vals in g:
                col.extend(int(c) for c in cols); val.extend(float(v) for v in vals)
                row_ptr.append(len(col))
            group_ptr.append(len(row_ptr) - 1)
        gp, rp, cc, vv = np.asarray(group_ptr, np.int64), np.asarray(row_ptr, np.int64), np.asarray(col, np.int32), np.asarray(val, np.float64)
        pr = _i(pairs).reshape(-1, 2)
        ga, gb = np.ascontiguousarray(pr[:, 0]), np.ascontiguousarray(pr[:, 1])
        out = np.zeros((len(pr), 36))
        _check(self.lib.pgo_sparse_chol_inverse_blocks(self.h, len(groups), gp.ctypes.data_as(_lp), rp.ctypes.data_as(_lp), _p(cc, _ip), _p(vv, _dp), len(pr), _p(ga, _ip), _p(gb, _ip), _p(out, _dp)), self.h)
        dim = lambda g: len(groups[g])
        return [out[k, :dim(a) * dim(b)].reshape(dim(a), dim(b)).copy() for k, (a, b) in enumerate(pr)]

    def selected_inverse(self):
        """every tile of A^-1 in the pattern of the factor (Takahashi's recurrence), kept in the object until the next factor(); the factor itself is only read"""
        _check(self.lib.pgo_sparse_chol_selected_inverse(self.h), self.h)

    def selected_info(self):
        """launches and tile products of one selected_inverse(), bytes of its tile array, whether a selected inverse of the present factor exists"""
        info = np.zeros(4, np.int64)
        _check(self.lib.pgo_sparse_chol_selected_info(self.h, info.ctypes.data_as(_lp)), self.h)
        return dict(zip(SELECTED_INFO, [int(v) for v in info]))

    def selected_blocks(self, node_a, node_b):
        """the blocks of A^-1 with the rows of keyframe node_a[k] and the columns of keyframe node_b[k], from the selected inverse -> (blocks (k, 6, 6), in_pattern
        (k,) bool).  A keyframe outside the system: a zero block; a block not wholly in the factor's pattern: zeros and in_pattern False."""
        a, b = _i(node_a).reshape(-1), _i(node_b).reshape(-1)
        assert a.shape == b.shape
        out, flag = np.zeros((len(a), 6, 6)), np.zeros(len(a), np.uint8)
        _check(self.lib.pgo_sparse_chol_selected_blocks(self.h, len(a), _p(a, _ip), _p(b, _ip), _p(out, _dp), _p(flag, _bp)), self.h)
        return out, flag.astype(bool)

    def inverse_columns(self, col_nodes, row_nodes, col_index):
        """blocks of A^-1 between ANY keyframes, in the factor's pattern or not: block k has the rows of keyframe row_nodes[k] and the columns of keyframe
        col_nodes[col_index[k]] -> (k, 6, 6).  col_nodes: distinct keyframes; their unit columns are solved by both sweeps, 64 at a time per workgroup, in chunks where
        they exceed the workspace limit.  A keyframe outside the system, as row or column: a zero block."""
        cn, rn, ci = _i(col_nodes).reshape(-1), _i(row_nodes).reshape(-1), _i(col_index).reshape(-1)
        assert rn.shape == ci.shape
        out = np.zeros((len(rn), 6, 6))
        _check(self.lib.pgo_sparse_chol_inverse_columns(self.h, len(cn), _p(cn, _ip), len(rn), _p(rn, _ip), _p(ci, _ip), _p(out, _dp)), self.h)
        return out

    def columns_info(self):
        """of the last inverse_columns(): launches, tile products, bytes of the workspace, chunks"""
        info = np.zeros(4, np.int64)
        _check(self.lib.pgo_sparse_chol_columns_info(self.h, info.ctypes.data_as(_lp)), self.h)
        return dict(zip(COLUMNS_INFO, [int(v) for v in info]))

    def set_workspace_limit(self, nbytes):
        """the most the right-hand sides of one chunk of inverse_columns() may take; at least one panel (64 rows of 64 nt doubles)"""
        _check(self.lib.pgo_sparse_chol_set_workspace_limit(self.h, int(nbytes)), self.h)


class SparseLm:
    """pgo_sparse_lm: the exact LM step on a SparseCholesky's factor.  node_free: 0 for a constant keyframe; the edges in internal order (relative-pose in add order,
    then switchable).  F must stay open while this object is used; its factor is the damped system's after a step."""

    def __init__(self, F, node_free, rel_c1, rel_c2, sw_c1, sw_c2):
        self.lib, self.F = load(), F
        self.h = C.c_void_p()
        free = np.ascontiguousarray(node_free, dtype=np.uint8)
        rc1, rc2, sc1, sc2 = _i(rel_c1), _i(rel_c2), _i(sw_c1), _i(sw_c2)
        assert free.shape == (F.n_nodes,) and rc1.shape == rc2.shape and sc1.shape == sc2.shape
        self.n_nodes, self.n_rel, self.n_sw = F.n_nodes, len(rc1), len(sc1)
        _check(self.lib.pgo_sparse_lm_create(F.h, self.n_nodes, _p(free, _bp), self.n_rel, _p(rc1, _ip), _p(rc2, _ip), self.n_sw, _p(sc1, _ip), _p(sc2, _ip), C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.lib.pgo_sparse_lm_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_scale(self, diag, sw_hss, jacobi_scaling=True):
        """the Jacobi scale of a linearisation's diag (n_nodes, 6, 6) and sw_hss: at iteration 0 only.  jacobi_scaling=False: S = 1"""
        d, h = _d(diag), _d(sw_hss)
        assert d.size == 36 * self.n_nodes and h.size == self.n_sw
        _check(self.lib.pgo_sparse_lm_set_scale(self.h, _p(d, _dp) if jacobi_scaling else None, _p(h, _dp)), self.F.h)

    def step(self, diag, grad, offdiag, sw_c, sw_hss, sw_gs, radius, min_lm_diagonal=1e-6, max_lm_diagonal=1e32):
        """one exact LM step from Problem.normal_blocks()' arrays -> (delta_pose (n_nodes, 6), delta_sw (n_sw,), model_cost_change, |d|, factor milliseconds).
        PgoError(PGO_ERR_NUMERIC): a pivot is not > 0; the object takes the next step."""
        a = [_d(x) for x in (diag, grad, offdiag, sw_c, sw_hss, sw_gs)]
        assert [x.size for x in a] == [36 * self.n_nodes, 6 * self.n_nodes, 36 * (self.n_rel + self.n_sw), 12 * self.n_sw, self.n_sw, self.n_sw]
        dpose, dsw, out3 = np.zeros((self.n_nodes, 6)), np.zeros(self.n_sw), np.zeros(3)
        _check(self.lib.pgo_sparse_lm_step(self.h, *[_p(x, _dp) for x in a], radius, min_lm_diagonal, max_lm_diagonal, _p(dpose, _dp), _p(dsw, _dp), _p(out3, _dp)), self.F.h)
        return dpose, dsw, float(out3[0]), float(out3[1]), float(out3[2])

    def last_times(self):
        """HIP-event milliseconds of the last step: upload, damping + fill + right-hand side, factor, sweeps, back-substitution + model, download"""
        ms = np.zeros(6)
        _check(self.lib.pgo_sparse_lm_last_times(self.h, _p(ms, _dp)), self.F.h)
        return dict(zip(LM_TIMES, [float(v) for v in ms]))

    def solve(self, callbacks, n_switch, swe_index, quat, t, sw, options, user=None):
        """pgo_sparse_lm_solve -> (quat, t, sw, capi.Summary); callbacks: an LmCallbacks; options: a capi.Options; user: what the callbacks get as their first argument"""
        from . import capi
        q, tt, s = capi.Problem._state(quat, t, sw)
        idx = _i(swe_index)
        assert idx.size == self.n_sw and s.size == n_switch and q.size == 4 * self.n_nodes
        summ = capi.Summary()
        _check(self.lib.pgo_sparse_lm_solve(self.h, C.byref(callbacks), user, n_switch, _p(idx, _ip), _p(q, _dp), _p(tt, _dp), _p(s, _dp), C.cast(C.byref(options), C.c_void_p), C.cast(C.byref(summ), C.c_void_p)), self.F.h)
        return q, tt, s, summ


@dataclasses.dataclass
class Edges:
    """what covariance() has to know of a Problem's residual blocks, in the order they were added: the relative-pose edges' endpoints, the switchable edges' endpoints and
    switch indices, the keyframes with a regulariser, the constant keyframes"""
    rel_c1: np.ndarray
    rel_c2: np.ndarray
    sw_c1: np.ndarray
    sw_c2: np.ndarray
    sw_idx: np.ndarray
    constant: np.ndarray = dataclasses.field(default_factory=lambda: np.zeros(0, np.int32))
    reg_node: np.ndarray = dataclasses.field(default_factory=lambda: np.zeros(0, np.int32))

    @classmethod
    def from_graph(cls, g, switchable=True, constant=()):
        """of capi.problem_from_graph(g, switchable)"""
        none = np.zeros(0, np.int32)
        if switchable:
            return cls(_i(g.odom_c1), _i(g.odom_c2), _i(g.loop_c1), _i(g.loop_c2), np.arange(g.n_loops, dtype=np.int32), _i(constant), _i(g.reg_node))
        return cls(_i(np.concatenate([g.odom_c1, g.loop_c1])), _i(np.concatenate([g.odom_c2, g.loop_c2])), none, none, none, _i(constant), _i(g.reg_node))


def covariance(P, edges, quat, t, sw, pairs, ordering=ORDER_AUTO, device_id=None, timings=None):
    """Problem.covariance for graphs of any size: pairs = [(a, b), ...] of block ids — below n_nodes a keyframe (6 tangent entries), n_nodes + i the switch index i (1
    entry) — at the given point; a list of (d_a, d_b) arrays.  P: a capi.Problem on one GPU whose residual blocks `edges` describes.  The system is the undamped Schur
    complement of P's normal blocks, factored by SparseCholesky; a keyframe is six unit rows, switch e the row -c_e / h_e, and 1 / h_e is added to a switch's variance.
    Pairs with a constant keyframe: zero blocks.  ValueError: an unreferenced keyframe or an unused switch.  PgoError(PGO_ERR_NUMERIC): the system is not positive
    definite (is the gauge fixed?) or a requested switch's h is not a positive finite number.  timings (a dict): HIP-event milliseconds of the factor and the blocks."""
    q = np.asarray(quat, dtype=np.float64).reshape(-1, 4)
    N = len(q)
    S = 0 if sw is None else int(np.asarray(sw).size)
    pr = _i(pairs).reshape(-1, 2)
    free = np.ones(N, np.uint8); free[np.asarray(edges.constant, dtype=np.int64)] = 0
    referenced = np.zeros(N, bool)
    for c in (edges.rel_c1, edges.rel_c2, edges.sw_c1, edges.sw_c2, edges.reg_node):
        referenced[np.asarray(c, dtype=np.int64)] = True
    edge_of = {int(s): e for e, s in enumerate(edges.sw_idx)}      # switch index -> the (last) switchable edge that uses it
    for i in np.unique(pr):
        if i < 0 or i >= N + S:
            raise ValueError("block id %d out of range (keyframes 0 .. n_nodes - 1, then n_nodes + switch index)" % i)
        if i < N and not referenced[i]:
            raise ValueError("keyframe %d is referenced by no residual block: it has no covariance" % i)
        if i >= N and int(i) - N not in edge_of:
            raise ValueError("switch %d is used by no switchable edge: it has no covariance" % (i - N))
    P.evaluate(quat, t, sw, want_residuals=False, want_gradient=True)
    diag, _, off, c, hss, _ = P.normal_blocks()
    dim = lambda i: 6 if i < N else 1
    is_const = lambda i: i < N and not free[i]
    live = [k for k, (a, b) in enumerate(pr) if not is_const(a) and not is_const(b)]
    out = [np.zeros((dim(a), dim(b))) for a, b in pr]
    if not live:
        return out
    ids = sorted({int(i) for k in live for i in pr[k]})
    for i in ids:
        if i >= N:
            h = hss[edge_of[i - N]]
            if not (h > 0.0 and np.isfinite(h)):
                raise PgoError(ERR_NUMERIC, "switch %d: J_s^T J_s = %r is not a positive finite number" % (i - N, h))
    in_system = (free != 0) & referenced
    hi, lo, sd, sb = reduce_normal_blocks(N, free, diag, off, c, hss, edges.rel_c1, edges.rel_c2, edges.sw_c1, edges.sw_c2)

    def rows_of(i):
        if i < N:
            return [([6 * i + a], [1.0]) for a in range(6)]
        e = edge_of[i - N]
        ends = sorted((int(n), side) for side, n in enumerate((edges.sw_c1[e], edges.sw_c2[e])) if free[n])      # (columns ascending; a constant end has no row in the system)
        return [([6 * n + a for n, _ in ends for a in range(6)], [-c[e, 6 * side + a] / hss[e] for _, side in ends for a in range(6)])]

    F = SparseCholesky(N, in_system, hi, lo, ordering, P.options.device_id if device_id is None else device_id)
    try:
        F.factor(sd, sb)
        if timings is not None:
            timings["factor_ms"] = F.last_ms(); timings["blocks_ms"] = 0.0; timings["info"] = F.info()[0]
        # at most MAX_GROUPS groups per call: pairs are served by the call that holds both their ids; the ids are dealt out in runs of MAX_GROUPS / 2
        half = MAX_GROUPS // 2
        runs = [ids[s:s + half] for s in range(0, len(ids), half)]
        run_of = {i: r for r, run in enumerate(runs) for i in run}
        todo = {}
        for k in live:
            a, b = int(pr[k][0]), int(pr[k][1])
            todo.setdefault(tuple(sorted({run_of[a], run_of[b]})), []).append(k)
        for key in sorted(todo):
            members = [i for r in key for i in runs[r]]
            at = {i: g for g, i in enumerate(members)}
            blocks = F.inverse_blocks([rows_of(i) for i in members], [(at[int(pr[k][0])], at[int(pr[k][1])]) for k in todo[key]])
            if timings is not None:
                timings["blocks_ms"] += F.last_ms()
            for k, blk in zip(todo[key], blocks):
                a, b = int(pr[k][0]), int(pr[k][1])
                if a >= N and a == b:
                    blk = blk + 1.0 / hss[edge_of[a - N]]
                out[k] = blk
    finally:
        F.close()
    return out


def handle_callbacks(P, hooks=None):
    """LmCallbacks over a capi.Problem: ctypes wrappers of P.evaluate, P.normal_blocks and P.manifold_plus that hand the solve's host pointers straight to
    pgo_evaluate, pgo_get_normal_blocks and pgo_manifold_plus.  hooks (a dict, optional): "normal_blocks": called as f(call index, diag (N, 6, 6), grad, offdiag,
    sw_c, sw_hss, sw_gs) on writable views after every fetch — tests disturb a linearisation through it.  No exception crosses the C boundary: it is printed and the
    callback returns PGO_ERR_INVALID_ARG."""
    hooks = hooks or {}
    calls = {"normal_blocks": 0}

    def guarded(f):
        def g(*a):
            try:
                return int(f(*a))
            except Exception:
                import traceback
                traceback.print_exc()
                return ERR_INVALID_ARG
        return g

    def evaluate(user, q, t, sw, n_nodes, n_switch, cost, res, grad):
        P._shape = (int(n_nodes), int(n_switch))
        return P.lib.pgo_evaluate(P.h, q, t, sw, C.c_int64(n_nodes), C.c_int64(n_switch), cost, res, grad)

    def normal_blocks(user, diag, grad, off, c, hss, gs):
        rc = P.lib.pgo_get_normal_blocks(P.h, diag, grad, off, c, hss, gs)
        if rc == 0 and "normal_blocks" in hooks:
            N, _ = P._shape
            view = lambda p, shape: np.ctypeslib.as_array(p, shape=shape) if p else None
            hooks["normal_blocks"](calls["normal_blocks"], view(diag, (N, 6, 6)), view(grad, (N, 6)), view(off, (P.n_rel + P.n_sw, 6, 6)), view(c, (P.n_sw, 12)), view(hss, (P.n_sw,)), view(gs, (P.n_sw,)))
        calls["normal_blocks"] += 1
        return rc

    def manifold_plus(user, n, q, t, d, qo, to):
        return P.lib.pgo_manifold_plus(P.h, C.c_int64(n), q, t, d, qo, to)

    return LmCallbacks(EVALUATE_FN(guarded(evaluate)), NORMAL_BLOCKS_FN(guarded(normal_blocks)), MANIFOLD_PLUS_FN(guarded(manifold_plus)))


def _refuse_busy_handle(P, n_nodes):
    """PgoError(PGO_ERR_STATE) for a handle inside an open solve or with a communicator attached: pgo_get_linear_solution names both states before it does anything"""
    x = np.zeros(6 * n_nodes)
    rc = P.lib.pgo_get_linear_solution(P.h, _p(x, _dp))
    text = P.lib.pgo_last_error(P.h).decode()
    if rc == ERR_STATE and "communicator" in text:
        raise PgoError(ERR_STATE, "solve_exact: one GPU only: a communicator is attached to the handle")
    if not (rc == ERR_STATE and "needs an open solve" in text):
        raise PgoError(ERR_STATE, "solve_exact inside a solve of the handle (between solve_begin and solve_end)")


def solve_exact(P, edges, quat, t, sw, ordering=ORDER_AUTO, device_id=None, timings=None, hooks=None, **options):
    """Problem.solve with every LM step exact, for graphs of any size: Ceres' trust-region solve on the tile-sparse Cholesky factor of every damped system —
    what linear_solver = LINEAR_DENSE_CHOLESKY gives up to DENSE_MAX_KEYFRAMES keyframes -> (quat, t, sw, capi.Summary); the inputs are not modified.
    P: a capi.Problem of any linear_solver on one GPU whose residual blocks `edges` describes; it linearises (evaluate, normal_blocks) and steps on the manifold
    (manifold_plus), its own solver does not run and its summary and trust-region state stay what they were.  options: fields of capi.Options that replace P's for
    this solve (max_num_iterations, function_tolerance, initial_trust_region_radius, ...).  PgoError(PGO_ERR_STATE): P is inside an open solve or has a communicator.
    timings (a dict): the plan's figures and the HIP-event milliseconds of the last step's phases (LM_TIMES)."""
    from . import capi
    q, tt, s = capi.Problem._state(quat, t, sw)
    N, S = q.size // 4, s.size
    _refuse_busy_handle(P, N)
    o = capi.Options.from_buffer_copy(P.options)
    for k, v in options.items():
        if not hasattr(o, k):
            raise TypeError("unknown option %r" % k)
        setattr(o, k, v)
    free = np.ones(N, np.uint8); free[np.asarray(edges.constant, dtype=np.int64)] = 0
    referenced = np.zeros(N, bool)
    for c in (edges.rel_c1, edges.rel_c2, edges.sw_c1, edges.sw_c2, edges.reg_node):
        referenced[np.asarray(c, dtype=np.int64)] = True
    in_system = (free != 0) & referenced
    ends = np.concatenate([np.stack([_i(edges.rel_c1), _i(edges.rel_c2)], axis=1), np.stack([_i(edges.sw_c1), _i(edges.sw_c2)], axis=1)]).astype(np.int64)
    ends = ends[(ends[:, 0] != ends[:, 1]) & in_system[ends[:, 0]] & in_system[ends[:, 1]]]
    pairs = np.unique(np.stack([ends.max(axis=1), ends.min(axis=1)], axis=1), axis=0) if len(ends) else np.zeros((0, 2), np.int64)
    F = SparseCholesky(N, in_system, pairs[:, 0], pairs[:, 1], ordering, P.options.device_id if device_id is None else device_id)
    try:
        L = SparseLm(F, free, edges.rel_c1, edges.rel_c2, edges.sw_c1, edges.sw_c2)
        try:
            cb = handle_callbacks(P, hooks)
            out = L.solve(cb, S, edges.sw_idx, q, tt, s, o)
            if timings is not None:
                timings["info"] = F.info()[0]; timings.update(L.last_times())
        finally:
            L.close()
    finally:
        F.close()
    return out


GRAPH_TIMES = ("upload_ms", "blocks_ms", "nodes_ms", "download_ms")      # pgo_sparse_graph_last_times
REFERENCE_YPR_GAINS = (4.0, 10.0, 10.0)                                   # the reference's FourDOFError, src/CeresResidues.h:303-305
_LOSSES = {None: 0, "huber": 1, "cauchy": 2}                              # PGO_LOSS_*


def _loss(loss):
    """None / ("huber", a) / ("cauchy", a) -> (PGO_LOSS_*, a); an unknown name goes through as an unknown code"""
    if loss is None:
        return 0, 0.0
    kind, a = loss
    return _LOSSES.get(kind, 99) if not isinstance(kind, int) else kind, float(a)


class Graph:
    """pgo_sparse_graph: a pose graph that linearises itself on the GPU — relative-pose, switchable and regulariser blocks, SixDOFError or yaw/pitch/roll-weighted
    (gains = three numbers > 0 per edge; the reference's are REFERENCE_YPR_GAINS), plain or robust — without a capi.Problem.  Add blocks, finalize(), then evaluate /
    normal_blocks / jacobian_blocks / manifold_plus have the contracts and orders of capi.Problem's; solve_graph() runs the exact LM solve on it."""

    def __init__(self, n_nodes, device_id=0):
        self.lib = load()
        self.h = C.c_void_p()
        self.n_nodes, self.n_rel, self.n_sw, self.n_reg = int(n_nodes), 0, 0, 0
        self.device_id = device_id
        _check(self.lib.pgo_sparse_graph_create(self.n_nodes, device_id, C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.lib.pgo_sparse_graph_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _gains(gains, n):
        if gains is None:
            return None
        return _d(np.broadcast_to(np.asarray(gains, dtype=np.float64).reshape(-1, 3), (n, 3)))

    def add_relpose_edges(self, c1, c2, c1_T_c2, weight, gains=None, loss=None):
        """gains: None (SixDOFError), three numbers for every edge, or (n, 3); loss: None, ("huber", a) or ("cauchy", a)"""
        a, b, T, w = _i(c1), _i(c2), _d(c1_T_c2).reshape(-1, 16), _d(weight)
        n = len(a)
        assert b.shape == (n,) and T.shape == (n, 16) and w.shape == (n,)
        g = self._gains(gains, n)
        kind, la = _loss(loss)
        _check(self.lib.pgo_sparse_graph_add_relpose_edges(self.h, n, _p(a, _ip), _p(b, _ip), _p(T, _dp), _p(w, _dp), None if g is None else _p(g, _dp), kind, la))
        self.n_rel += n

    def add_switchable_edges(self, c1, c2, c1_T_c2, switch_idx, gains=None, loss=None):
        a, b, T, idx = _i(c1), _i(c2), _d(c1_T_c2).reshape(-1, 16), _i(switch_idx)
        n = len(a)
        assert b.shape == (n,) and T.shape == (n, 16) and idx.shape == (n,)
        g = self._gains(gains, n)
        kind, la = _loss(loss)
        _check(self.lib.pgo_sparse_graph_add_switchable_edges(self.h, n, _p(a, _ip), _p(b, _ip), _p(T, _dp), _p(idx, _ip), None if g is None else _p(g, _dp), kind, la))
        self.n_sw += n

    def set_node_regularizers(self, node, target, weight):
        """REPLACES the regulariser set"""
        nd, T, w = _i(node), _d(target).reshape(-1, 16), _d(weight)
        assert T.shape == (len(nd), 16) and w.shape == (len(nd),)
        _check(self.lib.pgo_sparse_graph_set_node_regularizers(self.h, len(nd), _p(nd, _ip), _p(T, _dp), _p(w, _dp)))
        self.n_reg = len(nd)

    def set_nodes_constant(self, node):
        nd = _i(node)
        _check(self.lib.pgo_sparse_graph_set_nodes_constant(self.h, len(nd), _p(nd, _ip)))

    def finalize(self):
        """builds and uploads the tables; no launch"""
        _check(self.lib.pgo_sparse_graph_finalize(self.h))

    @classmethod
    def from_pose_graph(cls, g, switchable, loop_gains=None, odom_gains=None, loop_loss=None, constant=(), device_id=0):
        """capi.problem_from_graph(g, switchable, loop_loss=loop_loss) as a finalised Graph: odometry -> relative-pose edges (odom_gains), loop closures -> switchable
        edges with switch e on loop e, or relative-pose edges (loop_gains, loop_loss), the regularisers, the constant keyframes"""
        G = cls(g.n_poses, device_id)
        try:
            if g.n_odom:
                G.add_relpose_edges(g.odom_c1, g.odom_c2, g.odom_T, g.odom_w, odom_gains)
            if g.n_loops:
                if switchable:
                    G.add_switchable_edges(g.loop_c1, g.loop_c2, g.loop_T, np.arange(g.n_loops, dtype=np.int32), loop_gains, loop_loss)
                else:
                    G.add_relpose_edges(g.loop_c1, g.loop_c2, g.loop_T, g.loop_w, loop_gains, loop_loss)
            if len(g.reg_node):
                G.set_node_regularizers(g.reg_node, g.reg_T, g.reg_w)
            if len(constant):
                G.set_nodes_constant(constant)
            G.finalize()
        except Exception:
            G.close()
            raise
        return G

    def evaluate(self, quat, t, sw=None, want_residuals=True, want_gradient=True):
        """capi.Problem.evaluate -> (cost, residuals or None, gradient or None)"""
        from . import capi
        q, tt, s = capi.Problem._state(quat, t, sw)
        N, S = q.size // 4, s.size
        cost = C.c_double(0)
        res = np.zeros(6 * self.n_rel + 7 * self.n_sw + 6 * self.n_reg) if want_residuals else None
        grad = np.zeros(6 * N + S) if want_gradient else None
        _check(self.lib.pgo_sparse_graph_evaluate(self.h, _p(q, _dp), _p(tt, _dp), _p(s, _dp), N, S, C.byref(cost), None if res is None else res.ctypes.data_as(_dp),
                                                  None if grad is None else grad.ctypes.data_as(_dp)))
        return cost.value, res, grad

    def normal_blocks(self):
        """capi.Problem.normal_blocks of the last evaluation with a gradient -> (diag (N, 6, 6), grad (N, 6), offdiag (E, 6, 6), sw_c (n_sw, 12), sw_hss, sw_gs)"""
        N, E = self.n_nodes, self.n_rel + self.n_sw
        diag, grad, off = np.zeros((N, 6, 6)), np.zeros((N, 6)), np.zeros((E, 6, 6))
        c, hss, gs = np.zeros((self.n_sw, 12)), np.zeros(self.n_sw), np.zeros(self.n_sw)
        _check(self.lib.pgo_sparse_graph_normal_blocks(self.h, *[_p(a, _dp) for a in (diag, grad, off, c, hss, gs)]))
        return diag, grad, off, c, hss, gs

    def jacobian_blocks(self, kind, first=0, count=None):
        """capi.Problem.jacobian_blocks: kind 0 relative-pose, 1 switchable, 2 regulariser -> (J1, J2, dr_ds)"""
        n = [self.n_rel, self.n_sw, self.n_reg][kind] if 0 <= kind <= 2 else 0
        count = n - first if count is None else count
        J1, J2, ds = np.zeros((max(count, 0), 6, 6)), np.zeros((max(count, 0), 6, 6)), np.zeros((max(count, 0), 7))
        _check(self.lib.pgo_sparse_graph_jacobian_blocks(self.h, kind, first, count, _p(J1, _dp), _p(J2, _dp), _p(ds, _dp)))
        return J1, J2, ds

    def manifold_plus(self, quat, t, delta):
        q, tt, d = _d(quat).reshape(-1), _d(t).reshape(-1), _d(delta).reshape(-1)
        n = q.size // 4
        assert tt.size == 3 * n and d.size == 6 * n
        qo, to = np.zeros(4 * n), np.zeros(3 * n)
        _check(self.lib.pgo_sparse_graph_manifold_plus(self.h, n, _p(q, _dp), _p(tt, _dp), _p(d, _dp), _p(qo, _dp), _p(to, _dp)))
        return qo.reshape(-1, 4), to.reshape(-1, 3)

    def lm_callbacks(self):
        """(LmCallbacks, user) for SparseLm.solve: this graph's evaluate, normal_blocks and manifold_plus, called from C without a Python frame in between"""
        cb, user = LmCallbacks(), C.c_void_p()
        _check(self.lib.pgo_sparse_graph_lm_callbacks(self.h, C.byref(cb), C.byref(user)))
        return cb, user

    def edge_lists(self):
        """of a finalised graph: a dict of node_free, in_system, rel_c1, rel_c2, sw_c1, sw_c2, sw_idx, pair_hi, pair_lo and n_switch (the least the state must have)"""
        cnt = np.zeros(6, np.int64)
        _check(self.lib.pgo_sparse_graph_edge_lists(self.h, _p(cnt, _lp), None, None, *([None] * 7)))
        N, n_rel, n_sw, n_pairs, n_switch, _ = [int(v) for v in cnt]
        free, ins = np.zeros(N, np.uint8), np.zeros(N, np.uint8)
        names = ("rel_c1", "rel_c2", "sw_c1", "sw_c2", "sw_idx", "pair_hi", "pair_lo")
        arrays = [np.zeros(k, np.int32) for k in (n_rel, n_rel, n_sw, n_sw, n_sw, n_pairs, n_pairs)]
        _check(self.lib.pgo_sparse_graph_edge_lists(self.h, None, _p(free, _bp), _p(ins, _bp), *[_p(a, _ip) for a in arrays]))
        out = dict(zip(names, arrays))
        out.update(node_free=free, in_system=ins, n_switch=n_switch)
        return out

    def last_times(self):
        """HIP-event milliseconds of the last evaluate: upload of the state, block kernel + cost reduction, node kernel, download"""
        ms = np.zeros(4)
        _check(self.lib.pgo_sparse_graph_last_times(self.h, _p(ms, _dp)))
        return dict(zip(GRAPH_TIMES, [float(v) for v in ms]))


def solve_graph(G, quat, t, sw, ordering=ORDER_AUTO, timings=None, **options):
    """solve_exact with a Graph's own linearisation in place of a handle's: Ceres' trust-region solve with every step exact, for graphs of any size and with
    yaw/pitch/roll-weighted edges -> (quat, t, sw, capi.Summary); the inputs are not modified.  SparseCholesky and SparseLm are made from G's edge lists, on G's
    device; options: fields of a default capi.Options (max_num_iterations, function_tolerance, ...)."""
    from . import capi
    q, tt, s = capi.Problem._state(quat, t, sw)
    o = capi.default_options(**options)
    e = G.edge_lists()
    F = SparseCholesky(G.n_nodes, e["in_system"], e["pair_hi"], e["pair_lo"], ordering, G.device_id)
    try:
        L = SparseLm(F, e["node_free"], e["rel_c1"], e["rel_c2"], e["sw_c1"], e["sw_c2"])
        try:
            cb, user = G.lm_callbacks()
            out = L.solve(cb, s.size, e["sw_idx"], q, tt, s, o, user=user)
            if timings is not None:
                timings["info"] = F.info()[0]; timings.update(L.last_times())
        finally:
            L.close()
    finally:
        F.close()
    return out


def r2ypr(R):
    """the reference's R2ypr (src/utils/PoseManipUtils.cpp:143-158): yaw, pitch, roll of a rotation matrix, in degrees; R (..., 3, 3)"""
    R = np.asarray(R, dtype=np.float64)
    n, o, a = R[..., :, 0], R[..., :, 1], R[..., :, 2]
    y = np.arctan2(n[..., 1], n[..., 0])
    p = np.arctan2(-n[..., 2], n[..., 0] * np.cos(y) + n[..., 1] * np.sin(y))
    r = np.arctan2(a[..., 0] * np.sin(y) - a[..., 1] * np.cos(y), -o[..., 0] * np.sin(y) + o[..., 1] * np.cos(y))
    return np.stack([y, p, r], axis=-1) / np.pi * 180.0


def ypr2R(yaw, pitch, roll):
    """the reference's YawPitchRollToRotationMatrix (src/CeresResidues.h:458-476): Rz(yaw) Ry(pitch) Rx(roll), degrees -> (..., 3, 3)"""
    y, p, r = [np.asarray(x, dtype=np.float64) / 180.0 * np.pi for x in (yaw, pitch, roll)]
    cy, sy, cp, sp, cr, sr = np.cos(y), np.sin(y), np.cos(p), np.sin(p), np.cos(r), np.sin(r)
    rows = [[cy * cp, -sy * cr + cy * sp * sr, sy * sr + cy * sp * cr], [sy * cp, cy * cr + sy * sp * sr, -cy * sr + sy * sp * cr], [-sp, cp * sr, cp * cr]]
    return np.stack([np.stack(np.broadcast_arrays(*row), axis=-1) for row in rows], axis=-2)


def _quat_to_rot(q):
    x, y, z, w = np.moveaxis(np.asarray(q, dtype=np.float64), -1, 0)
    rows = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
            [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
    return np.stack([np.stack(row, axis=-1) for row in rows], axis=-2)


def yaw_state_to_poses(yaw, t, pitch, roll):
    """the 4-DoF state with every keyframe's constant pitch and roll (degrees) -> w_T_c (N, 4, 4)"""
    yaw, t = _d(yaw).reshape(-1), _d(t).reshape(-1, 3)
    T = np.tile(np.eye(4), (len(yaw), 1, 1))
    T[:, :3, :3] = ypr2R(yaw, _d(pitch).reshape(-1), _d(roll).reshape(-1))
    T[:, :3, 3] = t
    return T


def yaw_problem_from_pose_graph(g):
    """the arrays of YawGraph.from_pose_graph (see there), without a device: a dict of c1, c2, t_meas, rel_yaw, pitch_i, roll_i per edge (odometry, then loops) and
    yaw, t, pitch, roll per keyframe"""
    ypr = r2ypr(_quat_to_rot(g.init_q))
    c1 = np.concatenate([_i(g.odom_c1), _i(g.loop_c1)])
    c2 = np.concatenate([_i(g.odom_c2), _i(g.loop_c2)])
    T = np.concatenate([_d(g.odom_T).reshape(-1, 16), _d(g.loop_T).reshape(-1, 16)]).reshape(-1, 4, 4).transpose(0, 2, 1)      # column-major 16 -> (E, 4, 4)
    return dict(c1=c1, c2=c2, t_meas=_d(T[:, :3, 3]), rel_yaw=r2ypr(T[:, :3, :3])[:, 0].copy(), pitch_i=ypr[c1, 1].copy(), roll_i=ypr[c1, 2].copy(),
                yaw=ypr[:, 0].copy(), t=_d(g.init_t).reshape(-1, 3).copy(), pitch=ypr[:, 1].copy(), roll=ypr[:, 2].copy())


class YawGraph:
    """pgo_sparse_yaw_graph: the reference's 4-DoF pose graph (__USE_YPR_REP) that linearises itself on the GPU — every keyframe a yaw in DEGREES and a translation, every
    edge a QinFourDOFWeightError with the pitch and roll of its first keyframe as constants.  Add edges, finalize(), then evaluate / normal_blocks / jacobian_blocks /
    manifold_plus; solve_yaw_graph() runs the exact LM solve on it.  The state travels as (yaw (N,), t (N, 3)); the library's ambient layout (yaw in slot 0 of a
    keyframe's four quat slots, the others 0) and the tangent layout (N, 6) = [dyaw, 0, 0, dt] are include/pgo_sparse.h's."""

    def __init__(self, n_nodes, device_id=0):
        self.lib = load()
        self.h = C.c_void_p()
        self.n_nodes, self.n_edges = int(n_nodes), 0
        self.device_id = device_id
        _check(self.lib.pgo_sparse_yaw_graph_create(self.n_nodes, device_id, C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.lib.pgo_sparse_yaw_graph_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add_edges(self, c1, c2, t_meas, rel_yaw, pitch_i, roll_i, weight=None):
        """edge k from keyframe c1[k] (whose pitch and roll the record holds) to c2[k]; angles in degrees; weight None: 1, the reference's"""
        a, b, tm, ry, pi, ri = _i(c1), _i(c2), _d(t_meas).reshape(-1, 3), _d(rel_yaw), _d(pitch_i), _d(roll_i)
        n = len(a)
        w = None if weight is None else _d(weight)
        assert b.shape == (n,) and tm.shape == (n, 3) and ry.shape == (n,) and pi.shape == (n,) and ri.shape == (n,) and (w is None or w.shape == (n,))
        _check(self.lib.pgo_sparse_yaw_graph_add_edges(self.h, n, _p(a, _ip), _p(b, _ip), _p(tm, _dp), _p(ry, _dp), _p(pi, _dp), _p(ri, _dp), None if w is None else _p(w, _dp)))
        self.n_edges += n

    def set_nodes_constant(self, node):
        nd = _i(node)
        _check(self.lib.pgo_sparse_yaw_graph_set_nodes_constant(self.h, len(nd), _p(nd, _ip)))

    def finalize(self):
        """builds and uploads the tables; no launch"""
        _check(self.lib.pgo_sparse_yaw_graph_finalize(self.h))

    @classmethod
    def from_pose_graph(cls, g, constant=(0,), device_id=0):
        """The reference's 4-DoF problem of a graphgen.PoseGraph and its odometry poses (g.init_q, g.init_t) as a finalised YawGraph -> (G, yaw, t, pitch, roll): the
        start and every keyframe's constant pitch and roll, in degrees.  For every odometry and loop edge (c1, c2, c1_T_c2): t_meas = c1_T_c2[:3, 3], rel_yaw =
        R2ypr(c1_T_c2.R)[0], pitch_i, roll_i = R2ypr(w_T_c1.R)[1:] of the odometry pose of the edge's FIRST keyframe (src/PoseGraphSLAM.cpp:1608-1626).  The reference's
        loop-edge line (src/PoseGraphSLAM.cpp:1542) takes pitch and roll from the edge's other keyframe; this helper follows the functor's own definition (R_i is the
        rotation of the keyframe whose yaw and translation come first) and VINS-Fusion's.  Every weight is 1; constant: the keyframes held fixed (the gauge)."""
        p = yaw_problem_from_pose_graph(g)
        G = cls(g.n_poses, device_id)
        try:
            if len(p["c1"]):
                G.add_edges(p["c1"], p["c2"], p["t_meas"], p["rel_yaw"], p["pitch_i"], p["roll_i"])
            if len(constant):
                G.set_nodes_constant(constant)
            G.finalize()
        except Exception:
            G.close()
            raise
        return G, p["yaw"], p["t"], p["pitch"], p["roll"]

    @staticmethod
    def pack(yaw):
        """yaw (N,) -> the ambient quat array (N, 4): the yaw in slot 0, the others 0"""
        y = _d(yaw).reshape(-1)
        q = np.zeros((len(y), 4))
        q[:, 0] = y
        return q

    def evaluate(self, yaw, t, want_residuals=True, want_gradient=True):
        """-> (cost, residuals (4 E,) or None, gradient (6 N,) or None)"""
        q, tt = self.pack(yaw), _d(t).reshape(-1)
        N = len(q)
        assert tt.size == 3 * N
        cost = C.c_double(0)
        res = np.zeros(4 * self.n_edges) if want_residuals else None
        grad = np.zeros(6 * N) if want_gradient else None
        _check(self.lib.pgo_sparse_yaw_graph_evaluate(self.h, _p(q, _dp), _p(tt, _dp), N, C.byref(cost), None if res is None else res.ctypes.data_as(_dp),
                                                      None if grad is None else grad.ctypes.data_as(_dp)))
        return cost.value, res, grad

    def normal_blocks(self):
        """of the last evaluation with a gradient -> (diag (N, 6, 6), grad (N, 6), offdiag (E, 6, 6)); the pad rows and columns as include/pgo_sparse.h says"""
        diag, grad, off = np.zeros((self.n_nodes, 6, 6)), np.zeros((self.n_nodes, 6)), np.zeros((self.n_edges, 6, 6))
        _check(self.lib.pgo_sparse_yaw_graph_normal_blocks(self.h, *[_p(a, _dp) for a in (diag, grad, off)]))
        return diag, grad, off

    def jacobian_blocks(self, first=0, count=None):
        """-> (J1, J2) (count, 4, 4): rows r[0..3], columns [yaw, t] of the edge's first / second keyframe"""
        count = self.n_edges - first if count is None else count
        J1, J2 = np.zeros((max(count, 0), 4, 4)), np.zeros((max(count, 0), 4, 4))
        _check(self.lib.pgo_sparse_yaw_graph_jacobian_blocks(self.h, first, count, _p(J1, _dp), _p(J2, _dp)))
        return J1, J2

    def manifold_plus(self, yaw, t, delta):
        """delta (N, 6) = [dyaw, 0, 0, dt]; t None: the yaw alone -> (yaw, t or None)"""
        q, d = self.pack(yaw), _d(delta).reshape(-1)
        n = len(q)
        tt = None if t is None else _d(t).reshape(-1)
        assert d.size == 6 * n and (tt is None or tt.size == 3 * n)
        qo, to = np.zeros((n, 4)), None if tt is None else np.zeros(3 * n)
        _check(self.lib.pgo_sparse_yaw_graph_manifold_plus(self.h, n, _p(q, _dp), None if tt is None else _p(tt, _dp), _p(d, _dp), _p(qo, _dp), None if to is None else _p(to, _dp)))
        assert not qo[:, 1:].any()
        return qo[:, 0].copy(), None if to is None else to.reshape(-1, 3)

    def lm_callbacks(self):
        """(LmCallbacks, user) for SparseLm.solve: this graph's evaluate, normal_blocks and manifold_plus, called from C without a Python frame in between"""
        cb, user = LmCallbacks(), C.c_void_p()
        _check(self.lib.pgo_sparse_yaw_graph_lm_callbacks(self.h, C.byref(cb), C.byref(user)))
        return cb, user

    def edge_lists(self):
        """of a finalised graph: a dict of node_free, in_system, c1, c2, pair_hi, pair_lo"""
        cnt = np.zeros(3, np.int64)
        _check(self.lib.pgo_sparse_yaw_graph_edge_lists(self.h, _p(cnt, _lp), None, None, None, None, None, None))
        N, E, n_pairs = [int(v) for v in cnt]
        free, ins = np.zeros(N, np.uint8), np.zeros(N, np.uint8)
        arrays = [np.zeros(k, np.int32) for k in (E, E, n_pairs, n_pairs)]
        _check(self.lib.pgo_sparse_yaw_graph_edge_lists(self.h, None, _p(free, _bp), _p(ins, _bp), *[_p(a, _ip) for a in arrays]))
        out = dict(zip(("c1", "c2", "pair_hi", "pair_lo"), arrays))
        out.update(node_free=free, in_system=ins)
        return out

    def last_times(self):
        """HIP-event milliseconds of the last evaluate: upload of the state, block kernel + cost reduction, node kernel, download"""
        ms = np.zeros(4)
        _check(self.lib.pgo_sparse_yaw_graph_last_times(self.h, _p(ms, _dp)))
        return dict(zip(GRAPH_TIMES, [float(v) for v in ms]))


def solve_yaw_graph(G, yaw, t, ordering=ORDER_AUTO, timings=None, **options):
    """solve_graph over a YawGraph: Ceres' trust-region solve of the reference's 4-DoF problem with every step exact, for graphs of any size -> (yaw, t, capi.Summary);
    the inputs are not modified.  SparseCholesky and SparseLm are made from G's edge lists, on G's device (the factor works on 6 rows per keyframe, two of them identity
    rows); options: fields of a default capi.Options (max_num_iterations, function_tolerance, ...)."""
    from . import capi
    q, tt = G.pack(yaw), np.array(t, dtype=np.float64).reshape(-1).copy()
    assert tt.size == 3 * G.n_nodes and len(q) == G.n_nodes
    o = capi.default_options(**options)
    e = G.edge_lists()
    none = np.zeros(0, np.int32)
    F = SparseCholesky(G.n_nodes, e["in_system"], e["pair_hi"], e["pair_lo"], ordering, G.device_id)
    try:
        L = SparseLm(F, e["node_free"], e["c1"], e["c2"], none, none)
        try:
            cb, user = G.lm_callbacks()
            qo, to, _, summ = L.solve(cb, 0, none, q, tt, None, o, user=user)
            if timings is not None:
                timings["info"] = F.info()[0]; timings.update(L.last_times())
        finally:
            L.close()
    finally:
        F.close()
    qo = qo.reshape(-1, 4)
    assert not qo[:, 1:].any()
    return qo[:, 0].copy(), to.reshape(-1, 3), summ


@dataclasses.dataclass
class AllCovariances:
    """what covariance_all() returns; n_rel, n_sw: the relative-pose and the switchable edges in the order they were added"""
    pose: np.ndarray           # (N, 6, 6): every keyframe's marginal covariance; a constant keyframe: zeros; a keyframe referenced by no residual block: NaN
    rel_cross: np.ndarray      # (n_rel, 6, 6): cov(c1, c2) of every relative-pose edge, rows of c1
    sw_cross: np.ndarray       # (n_sw, 6, 6): cov(c1, c2) of every switchable edge, rows of c1
    switch_var: np.ndarray     # (n_sw,): the variance of every switchable edge's switch
    switch_pose: np.ndarray    # (n_sw, 2, 6): cov(switch e, keyframe c1), cov(switch e, keyframe c2)


def all_block_requests(n_nodes, edges):
    """(node_a, node_b) of the blocks covariance_all gathers: every keyframe with itself, then (c1, c2) of every relative-pose edge, then of every switchable edge —
    all of them blocks of the system, hence in the factor's pattern"""
    own = np.arange(n_nodes, dtype=np.int32)
    return _i(np.concatenate([own, _i(edges.rel_c1), _i(edges.sw_c1)])), _i(np.concatenate([own, _i(edges.rel_c2), _i(edges.sw_c2)]))


def assemble_all(n_nodes, in_system, referenced, edges, sw_c, sw_hss, blocks):
    """AllCovariances from the gathered blocks of all_block_requests (zero where a keyframe is outside the system), in fp64 numpy.  Switch e is the row v_e = -c_e / h_e
    on the edge's free endpoints: var = 1 / h_e + v_e^T Sigma v_e, cov(switch e, keyframe k) = v_c1^T Sigma(c1, k) + v_c2^T Sigma(c2, k) — all of it from the three
    blocks (c1, c1), (c1, c2), (c2, c2)."""
    N, n_rel, n_sw = n_nodes, len(edges.rel_c1), len(edges.sw_c1)
    blocks = np.asarray(blocks, dtype=np.float64).reshape(-1, 6, 6)
    assert len(blocks) == N + n_rel + n_sw
    ins = np.asarray(in_system).astype(bool)
    pose = blocks[:N].copy()
    pose[~np.asarray(referenced, dtype=bool)] = np.nan
    rel_cross, sw_cross = blocks[N:N + n_rel].copy(), blocks[N + n_rel:].copy()
    c1, c2 = np.asarray(edges.sw_c1, dtype=np.int64), np.asarray(edges.sw_c2, dtype=np.int64)
    c, h = _d(sw_c).reshape(n_sw, 12), _d(sw_hss).reshape(n_sw)
    v1 = np.where(ins[c1][:, None], -c[:, :6] / h[:, None], 0.0)
    v2 = np.where(ins[c2][:, None], -c[:, 6:] / h[:, None], 0.0)
    S11, S22, S12 = blocks[:N][c1], blocks[:N][c2], sw_cross
    quad = lambda u, S, w: np.einsum("ei,eij,ej->e", u, S, w)
    switch_var = 1.0 / h + (quad(v1, S11, v1) + 2.0 * quad(v1, S12, v2) + quad(v2, S22, v2))
    switch_pose = np.zeros((n_sw, 2, 6))
    switch_pose[:, 0] = np.einsum("ei,eij->ej", v1, S11) + np.einsum("ei,eji->ej", v2, S12)
    switch_pose[:, 1] = np.einsum("ei,eij->ej", v1, S12) + np.einsum("ei,eij->ej", v2, S22)
    return AllCovariances(pose, rel_cross, sw_cross, switch_var, switch_pose)


def covariance_all(P, edges, quat, t, sw, ordering=ORDER_AUTO, device_id=None, timings=None):
    """Every keyframe's marginal covariance and every edge's joint covariance (pose, pose, switch) at the given point, for graphs of any size: AllCovariances.  The
    linearisation, the reduction and the system are covariance()'s; instead of a forward sweep per requested row, one selected inverse (SparseCholesky.selected_inverse:
    about twice the factor's tile products, no dense array) and one gather of the N + n_rel + n_sw blocks; the switch quantities are formed on the host from them.
    This is an all-blocks call: a keyframe referenced by no residual block does not raise, its `pose` block is NaN; a constant keyframe's blocks are zero.
    PgoError(PGO_ERR_NUMERIC): the system is not positive definite (is the gauge fixed?), or some switchable edge's h is not a positive finite number.
    timings (a dict): HIP-event milliseconds of the factor, the selected inverse and the gather."""
    q = np.asarray(quat, dtype=np.float64).reshape(-1, 4)
    N = len(q)
    free = np.ones(N, np.uint8); free[np.asarray(edges.constant, dtype=np.int64)] = 0
    referenced = np.zeros(N, bool)
    for c in (edges.rel_c1, edges.rel_c2, edges.sw_c1, edges.sw_c2, edges.reg_node):
        referenced[np.asarray(c, dtype=np.int64)] = True
    P.evaluate(quat, t, sw, want_residuals=False, want_gradient=True)
    diag, _, off, c, hss, _ = P.normal_blocks()
    for e in range(len(edges.sw_c1)):
        if not (hss[e] > 0.0 and np.isfinite(hss[e])):
            raise PgoError(ERR_NUMERIC, "switch %d: J_s^T J_s = %r is not a positive finite number" % (int(edges.sw_idx[e]), hss[e]))
    in_system = (free != 0) & referenced
    hi, lo, sd, sb = reduce_normal_blocks(N, free, diag, off, c, hss, edges.rel_c1, edges.rel_c2, edges.sw_c1, edges.sw_c2)
    F = SparseCholesky(N, in_system, hi, lo, ordering, P.options.device_id if device_id is None else device_id)
    try:
        F.factor(sd, sb)
        if timings is not None:
            timings["factor_ms"] = F.last_ms(); timings["info"] = F.info()[0]
        F.selected_inverse()
        if timings is not None:
            timings["selected_ms"] = F.last_ms(); timings["selected_info"] = F.selected_info()
        na, nb = all_block_requests(N, edges)
        blocks, in_pattern = F.selected_blocks(na, nb)
        if timings is not None:
            timings["gather_ms"] = F.last_ms()
        if not in_pattern.all():      # (every request is a block of the system)
            k = int(np.flatnonzero(~in_pattern)[0])
            raise RuntimeError("covariance_all: the block of keyframes (%d, %d) is not in the factor's pattern" % (na[k], nb[k]))
    finally:
        F.close()
    return assemble_all(N, in_system, referenced, edges, c, hss, blocks)


def cross_blocks(F, pairs):
    """The blocks of A^-1 of any keyframe pairs [(a, b), ...] from F.inverse_columns (a SparseCholesky with a factor, or anything with that method) -> (n_pairs, 6, 6),
    rows of a, columns of b.  The column side — the keyframes whose unit columns are solved — is the side of the list with fewer distinct keyframes, the second elements
    on a tie.  Every block is gathered once: a pair asked again gets the same block, a pair asked the other way round its transpose, and a diagonal block is read
    once and its lower triangle mirrored — (b, a) is the exact transpose of (a, b), (a, a) exactly symmetric."""
    pr = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    out = np.zeros((len(pr), 6, 6))
    if not len(pr):
        return out
    side = 0 if len(np.unique(pr[:, 0])) < len(np.unique(pr[:, 1])) else 1
    cols = np.unique(pr[:, side])
    col_at = {int(c): k for k, c in enumerate(cols)}
    asked, rows, cidx = {}, [], []      # (row keyframe, column keyframe) -> index of the request
    take = []                           # per pair: (request, transposed)
    for a, b in pr:
        a, b = int(a), int(b)
        if (a, b) in asked:
            take.append((asked[(a, b)], False))
        elif (b, a) in asked:
            take.append((asked[(b, a)], True))
        else:
            r, c, tr = (a, b, False) if side == 1 else (b, a, True)
            asked[(r, c)] = len(rows); rows.append(r); cidx.append(col_at[c])
            take.append((asked[(r, c)], tr))
    got = F.inverse_columns(cols, rows, cidx)
    for (r, c), k in asked.items():
        if r == c:
            got[k] = np.tril(got[k]) + np.tril(got[k], -1).T
    for k, (q, tr) in enumerate(take):
        out[k] = got[q].T if tr else got[q]
    return out


SOLVE_BELOW_COLUMNS = 100      # see _Routed


class _Routed:
    """inverse_columns of a SparseCholesky for cross_blocks, with the measured rule: a request with fewer than SOLVE_BELOW_COLUMNS column keyframes goes to
    SparseCholesky.solve of their unit columns.  The panel sweeps pay a chain of 2 nt launches whose steps walk the tiles of a row one after the other in one workgroup
    per 64 right-hand sides, whatever the number of right-hand sides; the solve pays per right-hand side.  profiles/sparse_panel_solve_times.txt (HIP events; 1 100,
    3 000 and 10 000 keyframes, both orders): at 6, 60, 150 and 300 right-hand sides the solve takes 0.06 - 1.00 x the panel sweeps' time (300: 0.62 - 1.00), at 600
    it takes 1.19 - 1.60 x, at 6 000 4.8 - 14.7 x.  The two meet between 300 and 600 right-hand sides — 50 and 100 keyframes; 100 is the first measured count at which
    the panel sweeps win on every graph and order.  `ms`: HIP-event milliseconds of the calls; `route`: what served the last one."""

    def __init__(self, F):
        self.F, self.ms, self.route = F, 0.0, None

    def inverse_columns(self, col_nodes, row_nodes, col_index):
        cn, rn, ci = _i(col_nodes).reshape(-1), _i(row_nodes).reshape(-1), _i(col_index).reshape(-1)
        if len(cn) >= SOLVE_BELOW_COLUMNS:
            out = self.F.inverse_columns(cn, rn, ci)
            self.route = "columns"
        else:
            B = np.zeros((6 * len(cn), 6 * self.F.n_nodes))
            B[np.arange(6 * len(cn)), (6 * cn[:, None].astype(np.int64) + np.arange(6)).reshape(-1)] = 1.0
            X = self.F.solve(B).reshape(len(cn), 6, self.F.n_nodes, 6)      # [column keyframe, right-hand side j, row keyframe, entry i]
            out = np.ascontiguousarray(X[ci, :, rn, :].transpose(0, 2, 1))
            self.route = "solve"
        self.ms += self.F.last_ms()
        return out


def _pose_system(P, edges, quat, t, sw, nodes):
    """covariance()'s linearisation, checks and reduction for requests on keyframes alone: (N, in_system, pair_hi, pair_lo, s_diag, s_blocks)"""
    N = len(np.asarray(quat, dtype=np.float64).reshape(-1, 4))
    free = np.ones(N, np.uint8); free[np.asarray(edges.constant, dtype=np.int64)] = 0
    referenced = np.zeros(N, bool)
    for c in (edges.rel_c1, edges.rel_c2, edges.sw_c1, edges.sw_c2, edges.reg_node):
        referenced[np.asarray(c, dtype=np.int64)] = True
    for i in np.unique(np.asarray(nodes, dtype=np.int64)):
        if i < 0 or i >= N:
            raise ValueError("keyframe %d out of range (0 .. n_nodes - 1)" % i)
        if not referenced[i]:
            raise ValueError("keyframe %d is referenced by no residual block: it has no covariance" % i)
    P.evaluate(quat, t, sw, want_residuals=False, want_gradient=True)
    diag, _, off, c, hss, _ = P.normal_blocks()
    hi, lo, sd, sb = reduce_normal_blocks(N, free, diag, off, c, hss, edges.rel_c1, edges.rel_c2, edges.sw_c1, edges.sw_c2)
    return N, (free != 0) & referenced, hi, lo, sd, sb


def cross_covariance(P, edges, quat, t, sw, pairs, ordering=ORDER_AUTO, device_id=None, timings=None):
    """The 6 x 6 covariance blocks of ANY keyframe pairs [(a, b), ...], rows of a and columns of b, in any number -> (n_pairs, 6, 6): what covariance() gives for
    pairs of keyframes, for the blocks outside the factor's pattern too and without its limit of groups per call — the cross-covariances of loop-closure candidates.
    The linearisation, the reduction, the id checks and the rules are covariance()'s: a pair with a constant keyframe is a zero block, an unreferenced keyframe raises
    ValueError, PgoError(PGO_ERR_NUMERIC) a system that is not positive definite.  One factor, then cross_blocks (its rules on the column side and on transposes) on
    SparseCholesky.inverse_columns — or, below SOLVE_BELOW_COLUMNS column keyframes, on SparseCholesky.solve of their unit columns, which is measured faster there
    (_Routed).  timings (a dict): HIP-event milliseconds of the factor and the columns, and which of the two served them."""
    pr = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    N, in_system, hi, lo, sd, sb = _pose_system(P, edges, quat, t, sw, pr)
    F = SparseCholesky(N, in_system, hi, lo, ordering, P.options.device_id if device_id is None else device_id)
    try:
        F.factor(sd, sb)
        if timings is not None:
            timings["factor_ms"] = F.last_ms(); timings["info"] = F.info()[0]
        R = _Routed(F)
        out = cross_blocks(R, pr)
        if timings is not None:
            timings["columns_ms"] = R.ms; timings["route"] = R.route; timings["columns_info"] = F.columns_info()
    finally:
        F.close()
    return out


@dataclasses.dataclass
class LoopGate:
    """what loop_candidate_gate() returns, per candidate"""
    residual: np.ndarray           # (n, 6): the candidates' weighted residuals at the given point
    cross: np.ndarray              # (n, 6, 6): cov(c1, c2), rows of c1
    innovation_cov: np.ndarray     # (n, 6, 6): S, the covariance of the residual under the posterior plus its own unit noise
    mahalanobis2: np.ndarray       # (n,): d^2 = r^T S^-1 r — chi-square with 6 degrees of freedom for a true loop closure


def gate_from_blocks(r, J1, J2, S_aa, S_bb, S_ab):
    """the gate's arithmetic, in fp64 numpy: S = J1 S_aa J1^T + J1 S_ab J2^T + J2 S_ab^T J1^T + J2 S_bb J2^T + I per candidate (the residual is weighted: its noise is
    the identity), d^2 = r^T S^-1 r by a solve"""
    r, J1, J2 = _d(r).reshape(-1, 6), _d(J1).reshape(-1, 6, 6), _d(J2).reshape(-1, 6, 6)
    S_aa, S_bb, S_ab = _d(S_aa).reshape(-1, 6, 6), _d(S_bb).reshape(-1, 6, 6), _d(S_ab).reshape(-1, 6, 6)
    T = lambda M: M.transpose(0, 2, 1)
    cross = J1 @ S_ab @ T(J2)
    S = J1 @ S_aa @ T(J1) + cross + T(cross) + J2 @ S_bb @ T(J2) + np.eye(6)
    S = 0.5 * (S + T(S))      # (the two congruences round their two triangles apart)
    d2 = np.einsum("ei,ei->e", r, np.linalg.solve(S, r[:, :, None])[:, :, 0]) if len(r) else np.zeros(0)
    return LoopGate(r, S_ab, S, d2)


def loop_candidate_gate(P, edges, quat, t, sw, c1, c2, c1_T_c2, weight, ordering=ORDER_AUTO, device_id=None, timings=None):
    """The chi-square gate of loop-closure candidates: relative-pose edges (c1, c2, c1_T_c2, weight as add_relpose_edges takes them) that are NOT in the graph, judged
    under the posterior of the graph that is (P and `edges`, at the given point): LoopGate.  Residual and Jacobians come from a scratch capi.Problem with P's options
    that holds only the candidates — the tangent order and the weighting are the library's own; cov(c1, c1) and cov(c2, c2) come from the selected inverse, cov(c1, c2)
    through cross_covariance's
    path, on one factor.  A candidate between keyframes that are both constant has S = I.  Errors as cross_covariance's."""
    from . import capi
    c1, c2 = _i(c1).reshape(-1), _i(c2).reshape(-1)
    n = len(c1)
    assert len(c2) == n
    N, in_system, hi, lo, sd, sb = _pose_system(P, edges, quat, t, sw, np.concatenate([c1, c2]))
    scratch = capi.Problem(P.options)
    try:
        scratch.add_relpose_edges(c1, c2, c1_T_c2, weight)
        _, res, _ = scratch.evaluate(quat, t, None, want_residuals=True, want_gradient=True)
        J1, J2, _ = scratch.jacobian_blocks(0)
    finally:
        scratch.close()
    F = SparseCholesky(N, in_system, hi, lo, ordering, P.options.device_id if device_id is None else device_id)
    try:
        F.factor(sd, sb)
        if timings is not None:
            timings["factor_ms"] = F.last_ms(); timings["info"] = F.info()[0]
        F.selected_inverse()
        if timings is not None:
            timings["selected_ms"] = F.last_ms()
        own, in_pattern = F.selected_blocks(np.concatenate([c1, c2]), np.concatenate([c1, c2]))
        assert in_pattern.all()      # (diagonal blocks)
        R = _Routed(F)
        S_ab = cross_blocks(R, np.stack([c1, c2], axis=1))
        if timings is not None:
            timings["columns_ms"] = R.ms; timings["route"] = R.route; timings["columns_info"] = F.columns_info()
    finally:
        F.close()
    return gate_from_blocks(res.reshape(n, 6), J1, J2, own[:n], own[n:], S_ab)
