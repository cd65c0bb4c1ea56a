"""The calls whose returned bits tests/golden/sparse_kernel_bits.json records: what scripts/record_sparse_kernel_bits.py (which writes the file) and
tests/test_gpu_sparse_bits.py (which compares against it) share.  Small inputs, a few tiles each, on which the MFMA kernels of libpgo_sparse.so (sc_panel_kernel,
sc_update_kernel, sc_sel_ginv_kernel, sc_sel_column_kernel, sc_sel_diag_kernel, sc_pfwd_kernel, sc_pbwd_kernel: csrc/pgo_sparse_kernels.hpp) run in each of their
branches:

  spd_<matrix>, spd_<matrix>_perm   spd_solve on the matrices of tests/test_sparse_cholesky_host.CASES and GAP — one tile, padding, an empty s_0 (the diagonal tile as a
                                    step of its own), an arrow, a fill-only tile, bands, a gap — and on full200 (every tile stored: `ahead` in every step, the pair
                                    (0, 0) factored in LDS), in natural order and under one fixed permutation of the 6-row nodes;
  blocks40_natural, blocks40_rcm    the 40-keyframe system of tests/test_sparse_panel_host.gather_case through the block interface: factor and solve with 3 right-hand
                                    sides; selected_inverse and selected_blocks of EVERY ordered pair (a, b) — every in-pattern pair both ways round, so the column
                                    kernel reads tiles as stored and transposed; inverse_columns with 11 column keyframes (66 rows: two panels, a keyframe across the
                                    panel edge) whose columns and rows begin past the first tile (first > 0, k_stop > 0), again under a workspace limit of one panel (in
                                    chunks), and with columns and rows from the first tile on;
  lm24_natural, lm24_rcm            one SparseLm.step on a 24-keyframe chain of tests/sparse_lm_cases.py with switchable loops: dp, ds and the model cost change.

Every input is made of integers or of numpy's own generator and elementwise arithmetic, no BLAS product: the same doubles wherever they are built.  run(name) returns
(inputs, outputs): a list of arrays and a dict of arrays; digests(name) their sha256."""
import hashlib

import numpy as np

from solve_keyframe_pose_graph_amd import sparse_cholesky as sc
from tests import sparse_lm_cases as lc
from tests.pose_cov_cases import spd
from tests.test_sparse_cholesky_host import CASES, NB, patterned
from tests.test_sparse_companion_host import GAP
from tests.test_sparse_panel_host import GATHER_N, gather_case

MATRICES = dict(CASES, gap=GAP)
SPD = sorted(MATRICES) + ["full200"]
ORDERINGS = {"natural": sc.ORDER_NATURAL, "rcm": sc.ORDER_RCM}
COLUMN_NODES = list(range(15, 26))      # 11 keyframes, rows 90 .. 155 in natural order: past the first tile; right-hand side rows 60 .. 65 lie across the panel edge
ROW_NODES = list(range(12, 39))         # rows 72 .. in natural order: the backward sweep stops before tile 0
WIDE_COLUMNS = [0, 5, 10, 20, 30, 38]
LM_GRAPH = lambda: lc.chain(24, [(20, 2), (15, 4), (4, 15), (23, 11)], constant=(7,))
LM_RADIUS = 1e4

CASE_NAMES = tuple(["spd_" + m + s for m in SPD for s in ("", "_perm")] + ["blocks40_" + o for o in ORDERINGS] + ["lm24_" + o for o in ORDERINGS])


def spd_case(matrix, permuted):
    """(A, b, pos): the host tests' matrices (their seeds), cut to whole 6-row nodes where permuted; full200: pose_cov_cases.spd, integers"""
    n, tiles = (200, None) if matrix == "full200" else MATRICES[matrix][:2]
    if permuted:
        n = n // 6 * 6
    if tiles is None:
        A, b = spd(n), np.random.default_rng(n).standard_normal(n)
    else:
        A, b = patterned(n, tiles, n + 1 if permuted else n)
    pos = None
    if permuted:
        node_pos = np.random.default_rng(5).permutation(n // 6)
        pos = (6 * node_pos[:, None] + np.arange(6)[None, :]).reshape(-1).astype(np.int32)
    return np.ascontiguousarray(A), np.ascontiguousarray(b), pos


def run_spd(matrix, permuted):
    A, b, pos = spd_case(matrix, permuted)
    x, info, _ = sc.spd_solve(A, b, pos)
    assert info["nt"] == (len(b) + NB - 1) // NB
    return [A, b] + ([] if pos is None else [pos]), {"x": x}


def run_blocks40(ordering):
    ins, hi, lo, diag, blocks, _, _ = gather_case()
    N = GATHER_N
    B = np.random.default_rng(40).standard_normal((3, 6 * N))
    every = np.arange(N)
    na, nb = np.repeat(every, N), np.tile(every, N)
    cols, rows = np.asarray(COLUMN_NODES), np.asarray(ROW_NODES)
    rn, ci = np.repeat(rows, len(cols)), np.tile(np.arange(len(cols)), len(rows))
    wide = np.asarray(WIDE_COLUMNS)
    wrn, wci = np.repeat(every, len(wide)), np.tile(np.arange(len(wide)), N)
    out = {}
    F = sc.SparseCholesky(N, ins, hi, lo, ordering)
    F.factor(diag, blocks)
    nt = F.info()[0]["nt"]
    out["solve"] = F.solve(B)
    F.selected_inverse()
    out["selected_blocks"], flag = F.selected_blocks(na, nb)
    out["selected_in_pattern"] = flag.astype(np.uint8)
    out["columns"] = F.inverse_columns(cols, rn, ci)
    whole = F.columns_info()
    out["columns_wide"] = F.inverse_columns(wide, wrn, wci)
    F.set_workspace_limit(NB * NB * nt * 8)      # one panel
    out["columns_chunked"] = F.inverse_columns(cols, rn, ci)
    parts = F.columns_info()
    F.close()
    assert nt == 4 and flag.any() and whole["chunks"] == 1 and whole["bytes"] == 2 * NB * NB * nt * 8 and parts["chunks"] == 2      # two panels; one per chunk under the limit
    return [ins, hi, lo, diag, blocks, B, na, nb, cols, rn, ci, wide, wrn, wci], out


def integer_blocks(seed, N, rel, sw):
    """lc.jacobian_blocks with integer Jacobians and residuals in [-3, 3]: every sum of products below is exact, whatever computes it"""
    rng = np.random.default_rng(seed)
    n_rel, n_sw = len(rel), len(sw)
    ints = lambda *shape: rng.integers(-3, 4, shape).astype(np.float64)
    diag, grad = np.zeros((N, 6, 6)), np.zeros((N, 6))
    off, c, hss, gs = np.zeros((n_rel + n_sw, 6, 6)), np.zeros((n_sw, 12)), np.zeros(n_sw), np.zeros(n_sw)
    diag[0] += 4.0 * np.eye(6); grad[0] += ints(6)
    for e, (a, b) in enumerate(np.vstack([rel.reshape(-1, 2), sw.reshape(-1, 2)])):
        rows = 6 if e < n_rel else 7
        J1, J2, r = ints(rows, 6) + 4.0 * np.eye(rows, 6), ints(rows, 6) - 4.0 * np.eye(rows, 6), ints(rows)
        diag[a] += J1.T @ J1; diag[b] += J2.T @ J2; off[e] = J1.T @ J2
        grad[a] += J1.T @ r; grad[b] += J2.T @ r
        if e >= n_rel:
            Js = ints(7) + 4.0
            s = e - n_rel
            c[s, :6], c[s, 6:], hss[s], gs[s] = J1.T @ Js, J2.T @ Js, Js @ Js, Js @ r
    return lc.Blocks(diag, grad, off, c, hss, gs)


def run_lm24(ordering):
    N, free, rel, sw = LM_GRAPH()
    ins = lc.in_system_of(N, free, rel, sw)
    hi, lo = lc.pairs_of(ins, rel, sw)
    B = integer_blocks(24, N, rel, sw)
    F = sc.SparseCholesky(N, ins, hi, lo, ordering)
    L = sc.SparseLm(F, free, rel[:, 0], rel[:, 1], sw[:, 0], sw[:, 1])
    L.set_scale(B.diag, B.hss)
    dp, ds, model, _, _ = L.step(B.diag, B.grad, B.off, B.c, B.hss, B.gs, LM_RADIUS)
    L.close(); F.close()
    return [ins, free, hi, lo, rel, sw, B.diag, B.grad, B.off, B.c, B.hss, B.gs], {"delta_pose": dp, "delta_sw": ds, "model_cost_change": np.array([model])}


def run(name):
    kind, _, rest = name.partition("_")
    if kind == "spd":
        return run_spd(rest[:-5] if rest.endswith("_perm") else rest, rest.endswith("_perm"))
    return {"blocks40": run_blocks40, "lm24": run_lm24}[kind](ORDERINGS[rest])


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
