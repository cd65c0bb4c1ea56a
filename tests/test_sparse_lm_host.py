"""CPU: the host side of the exact LM step and solve of libpgo_sparse.so (csrc/pgo_sparse_lm_math.hpp) through tests/native/sparse_lm_host.cpp — the step plan, the damped
Schur complement and its right-hand side as the fill writes them into the permuted tiles, the whole step on ScHost, a failed pivot, and the solve loop (sc_lm_solve, the
one pgo_sparse_lm_solve runs) with scripted callbacks, its decisions replayed through tests/native/lm_host.cpp.  The kernels run on the GPU only
(tests/test_gpu_sparse_lm.py, which holds them to this host instantiation).

Bounds, derived, u = 2^-53, eps = 2 u.
 * An entry of the damped Schur complement is hd - sum_k p_k a_k (+ lambda on the diagonal), k Schur terms, summed in fp64 in list order.  A Schur term carries: the
   product p_k (u), the pivot a_k = 1 / (h + lambda) — lambda = clamp(s s h) / (r s s): five roundings, the sum one more and lambda's share of them, the reciprocal one:
   7 u — and the product with it (u): 9 u; lambda itself 5 u; the additions (k + 1) u of the partial sums, each at most the sum of the magnitudes `mag`.  With cnt the
   number of terms: |error| <= (cnt + 8) u mag <= (cnt + 5) eps mag — the form (count + constant) eps mag of tests/test_sparse_companion_host.py's reduction bound,
   the constant raised from 1 to 5 by the damping's roundings.  The right-hand side's entries: the same count.
 * eta(A, b, x) <= n u for the FULL damped system (pose rows and switches, n its order), tests/test_gpu_dense_cholesky.py's figure and derivation.
Every test prints its figures (`SPARSELM ...`) before it asserts."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from solve_keyframe_pose_graph_amd import _build
from tests import precond_cases as pc
from tests import sparse_lm_cases as lc
from tests.test_lm_controller import GXX as LM_GXX
from tests.test_lm_controller import MID, STATE, call, step_args
from tests.test_sparse_companion_host import host_reduce
from tests.test_sparse_companion_host import load_shim as load_companion_shim

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
U, EPS = lc.U, np.finfo(np.float64).eps
STEP_INVALID_FACTORIZATION, STEP_REJECTED_RHO, CONVERGENCE = 3, 1, 0


@pytest.fixture(scope="module")
def shim():
    return lc.load_shim()


GRAPHS = {
    "nine": lc.nine,
    "k11": lambda: lc.chain(11, [(9, 1)]),                          # 66 rows: two tiles, keyframe 10 straddles them
    "k22": lambda: lc.chain(22, [(20, 2), (15, 4), (4, 15)], constant=(7,)),
    "tl200": lambda: lc.from_pose_graph(pc.graph("tl200")),
}


# ---- 1. the plan
@pytest.mark.parametrize("ordering", [0, 1])
def test_the_plan_equals_a_brute_force_construction(shim, ordering):
    N, free, rel, sw = lc.nine()
    H, ins, hi, lo = lc.host_lm(shim, (N, free, rel, sw), ordering)
    got_ins, got = H.plan(len(hi))
    H.close()
    assert list(ins) == [1, 1, 1, 1, 0, 0, 1, 1, 0] and np.array_equal(got_ins, ins)      # constant in the middle, the last one unreferenced
    want = lc.brute_plan(N, ins, hi, lo, rel, sw)
    for name, a, b in zip(("side_ptr", "side", "pair_ptr", "pair_ent", "inc_ptr", "inc"), got, want):
        assert np.array_equal(a, b), name
    k = [i for i, (h, l) in enumerate(zip(hi, lo)) if {int(h), int(l)} == {1, 2}][0]
    assert got[2][k + 1] - got[2][k] == 3      # three edges on the pair (1, 2): relative-pose both ways, then the switchable one
    assert {int(e) & 1 for e in got[3][got[2][k]:got[2][k + 1]][:2]} == {0, 1}      # one of the two relative-pose edges is read transposed
    assert got[0][4] == got[0][5] == got[0][6] and got[4][8] == got[4][9]      # constant and unreferenced keyframes have empty lists
    print("SPARSELM plan nine ordering %d: %d switch sides, %d pair entries on %d pairs, %d incident sides" % (ordering, len(got[1]), len(got[3]), len(hi), len(got[5])))


def test_bad_plans_are_refused(shim):
    N, free, rel, sw = lc.nine()
    ins = lc.in_system_of(N, free, rel, sw)
    hi, lo = lc.pairs_of(ins, rel, sw)
    for bad_rel, what in ((np.vstack([rel, [(0, 3)]]), "no pair of the factor"), (np.vstack([rel, [(3, 3)]]), "with itself"), (np.vstack([rel, [(0, 9)]]), "out of range")):
        H = lc.HostLm(shim, N, ins, free, hi, lo, bad_rel, sw, 0)
        assert not H.h and what in H.error, H.error
    free2 = free.copy(); free2[8] = 1
    H = lc.HostLm(shim, N, ins, free2, hi, lo, np.vstack([rel[:-1], [(8, 7)]]), sw, 0)      # a free keyframe the factor keeps outside, touched by an edge
    assert not H.h and "outside the system" in H.error


# ---- 2. the system
@pytest.mark.parametrize("radius", pc.RADII)
@pytest.mark.parametrize("name", ["nine", "tl200"])
def test_the_damped_system_against_a_longdouble_assembly(shim, name, radius):
    N, free, rel, sw = graph = GRAPHS[name]()
    H, ins, hi, lo = lc.host_lm(shim, graph, 1)
    B = lc.jacobian_blocks(7, N, rel, sw)
    assert H.set_scale(B) == 0
    ok, A, b, lam, ai = H.system(B, radius)
    H.close()
    assert ok
    F = lc.full_system(N, ins, rel, sw, B, radius)
    S, rhs, mag, cnt, bmag, bcnt = lc.reduced(F)
    rows = F.rows
    err = np.abs(A[np.ix_(rows, rows)].astype(np.longdouble) - S).astype(np.float64)
    bound = ((cnt + 5) * EPS * mag).astype(np.float64)
    berr = np.abs(b[rows].astype(np.longdouble) - rhs).astype(np.float64)
    bbound = ((bcnt + 5) * EPS * bmag).astype(np.float64)
    worst = float((err / np.maximum(bound, 1e-300)).max()), float((berr / np.maximum(bbound, 1e-300)).max())
    print("SPARSELM system %-6s radius %.0e  n %d  up to %d terms per entry  worst error / bound: matrix %.3f, right-hand side %.3f" % (name, radius, len(rows), cnt.max(), *worst))
    assert np.all(err <= bound) and np.all(berr <= bbound)
    assert np.array_equal(A, A.T)
    outside = np.ones(6 * N, bool); outside[rows] = False
    assert np.array_equal(A[np.ix_(outside, outside)], np.eye(int(outside.sum()))) and not A[np.ix_(outside, rows)].any() and not b[outside].any()
    assert np.all(np.abs(lam[rows] - F.lam_p.reshape(-1)[rows].astype(np.float64)) <= 5 * U * lam[rows]) and not lam[outside].any()
    assert name != "nine" or cnt.max() >= 4      # several edges on one pair were summed


@pytest.mark.parametrize("name", ["nine", "tl200"])
def test_at_a_huge_radius_the_system_is_the_undamped_reduction_to_rounding(shim, name):
    """radius = 1e16, clamps (0, inf).  NOT as numbers: the damping left is lambda = H_jj / 1e16, about half an ulp of the diagonal entry it is added to — the one added
    term, which may or may not round away — and the switch term is a product with the reciprocal 1 / (h + h / 1e16), not pgo_sparse_reduce_normal_blocks' division by
    h.  To rounding: within the bound of the module's docstring around the undamped blocks, whose own error is (cnt + 1) eps mag (tests/test_sparse_companion_host.py)."""
    N, free, rel, sw = graph = GRAPHS[name]()
    H, ins, hi, lo = lc.host_lm(shim, graph, 0)
    B = lc.jacobian_blocks(3, N, rel, sw)
    H.set_scale(B)
    ok, A, b, lam, ai = H.system(B, 1e16, 0.0, np.inf)
    H.close()
    assert ok
    phi, plo, sd, sb = host_reduce(load_companion_shim(), N, free, B.diag, B.off, B.c, B.hss, rel, sw)
    F = lc.full_system(N, ins, rel, sw, B, 1e16, 0.0, np.inf)
    _, _, mag, cnt, _, _ = lc.reduced(F)
    at = {int(r): k for k, r in enumerate(F.rows)}
    worst, equal, total = 0.0, 0, 0
    blocks = [(i, i, sd[i]) for i in range(N) if ins[i]] + [(int(a), int(c), sb[k]) for k, (a, c) in enumerate(zip(phi, plo)) if ins[a] and ins[c]]
    for i, j, blk in blocks:
        got = A[6 * i:6 * i + 6, 6 * j:6 * j + 6]
        sel = np.ix_([at[6 * i + a] for a in range(6)], [at[6 * j + a] for a in range(6)])
        bound = ((2 * cnt[sel] + 6) * EPS * mag[sel]).astype(np.float64)      # both sides' bounds: (cnt + 5) + (cnt + 1)
        err = np.abs(got - blk)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        equal += int((got == blk).sum()); total += 36
        assert np.all(err <= bound), (i, j)
    print("SPARSELM undamped %-6s radius 1e16: %d of %d entries equal as numbers, worst difference / bound %.3f" % (name, equal, total, worst))


# ---- 3. the step
STEP_CASES = [("k11", 0), ("k11", 1), ("k22", 1), ("nine", 1), ("tl200", 0), ("tl200", 1)]


@pytest.mark.parametrize("radius", pc.RADII)
@pytest.mark.parametrize("name,ordering", STEP_CASES)
def test_the_step_solves_the_full_damped_system(shim, name, ordering, radius):
    N, free, rel, sw = graph = GRAPHS[name]()
    H, ins, hi, lo = lc.host_lm(shim, graph, ordering)
    B = lc.jacobian_blocks(11, N, rel, sw)
    H.set_scale(B)
    rc, d, s, out3 = H.step(B, radius)
    rc2, d2, s2, out32 = H.step(B, radius)
    sizes = H.sizes()[0]
    H.close()
    assert rc == 0 and rc2 == 0
    F = lc.full_system(N, ins, rel, sw, B, radius)
    x = F.vector(d, s)
    n = len(x)
    e = lc.eta(F.H, -F.g, x)
    want = lc.model_cost_change(F, x)
    rel_model = abs(out3[0] - want) / abs(want)
    print("SPARSELM step %-6s ordering %d radius %.0e  n %d (%d tiles of L in %d tile rows)  eta %.3e = %.2f u (bound n u = %.3e)  model cost change %.12e, relative error %.2e  |d| %.3e"
          % (name, sizes["ordering"], radius, n, sizes["l_tiles"], sizes["nt"], e, e / U, n * U, out3[0], rel_model, out3[1]))
    assert e <= n * U
    assert rel_model <= 1e-12
    assert abs(out3[1] - float(np.sqrt((x.astype(np.longdouble) ** 2).sum()))) <= 1e-14 * out3[1]
    outside = np.repeat(ins == 0, 6)
    assert not d.reshape(-1)[outside].any()
    assert np.array_equal(d, d2) and np.array_equal(s, s2) and out3[0] == out32[0]
    assert name != "k11" or sizes["nt"] == 2


# ---- 4. a failed pivot
def test_an_indefinite_block_is_reported_and_the_next_step_is_that_of_a_fresh_object(shim):
    N, free, rel, sw = graph = GRAPHS["k22"]()
    B = lc.jacobian_blocks(5, N, rel, sw)
    H, ins, hi, lo = lc.host_lm(shim, graph, 1)
    assert H.step(B, 1e4)[0] == lc.ERR_STATE      # no scale yet
    H.set_scale(B)
    bad = lc.Blocks(B.diag.copy(), B.grad, B.off, B.c, B.hss, B.gs)
    bad.diag[12] -= 200.0 * np.eye(6)
    rc, d, s, _ = H.step(bad, 1e4)
    assert rc == lc.ERR_NUMERIC and np.all(d == 7.0) and np.all(s == 7.0)      # nothing written
    neg = lc.Blocks(B.diag, B.grad, B.off, B.c, -B.hss, B.gs)
    assert H.step(neg, 1e4)[0] == lc.ERR_NUMERIC      # a damped switch pivot that is not > 0
    rc, d, s, out3 = H.step(B, 1e4)
    H.close()
    G, _, _, _ = lc.host_lm(shim, graph, 1)
    G.set_scale(B)
    rc2, d2, s2, out32 = G.step(B, 1e4)
    G.close()
    assert rc == 0 and rc2 == 0 and np.array_equal(d, d2) and np.array_equal(s, s2) and out3[0] == out32[0] and out3[1] == out32[1]


# ---- 5. the controller
LM_OPT = dict(max_num_iterations=50, max_num_consecutive_invalid_steps=5, initial_trust_region_radius=1e4, max_trust_region_radius=1e16, min_trust_region_radius=1e-32,
              min_relative_decrease=1e-3, function_tolerance=1e-6, gradient_tolerance=1e-10, parameter_tolerance=1e-8)


def scripted(shim, N, ordering, inflate=-1, fail_eval=-1, bad_lin=-1, **opt):
    o = dict(LM_OPT, **opt)
    v = np.array([o[k] for k in ("max_num_iterations", "max_num_consecutive_invalid_steps", "initial_trust_region_radius", "max_trust_region_radius", "min_trust_region_radius",
                                     "min_relative_decrease", "function_tolerance", "gradient_tolerance", "parameter_tolerance")] + [lc.MIN_DIAG, lc.MAX_DIAG, 1.0])
    t = np.full(3 * N, 0.25)
    rec, meta, msg = np.zeros((256, 9)), np.zeros(4), C.create_string_buffer(256)
    script = lc.I32([inflate, fail_eval, bad_lin])
    rc = shim.slh_scripted_solve(N, ordering, lc.P(script, lc.ip), lc.P(v, lc.dp), lc.P(t, lc.dp), lc.P(rec, lc.dp), lc.P(meta, lc.dp), msg)
    return rc, t, rec[:max(int(meta[0]), 0)], meta, msg.value.decode()


@pytest.fixture(scope="module")
def lm_shim():
    so = os.path.join(HERE, "native", "liblm_host.so")
    src = os.path.join(HERE, "native", "lm_host.cpp")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(os.path.join(lc.CSRC, "pgo_lm.hpp"))):
        subprocess.check_call(LM_GXX + ["-O2", "-fPIC", "-shared", "-o", so, src])
    return C.CDLL(so)


def replay(lm_shim, rec, opt):
    """every record through pgo_lm.hpp's decisions as tests/test_lm_controller.py drives them: the radius, the outcome and the relative decrease have to be the record's"""
    state = dict(zip(STATE, call(lm_shim, "begin", MID, opt, [])[0]))
    for k in range(1, len(rec)):
        valid, successful, reason, radius, rho, cost, model, norm, dcost = rec[k]
        assert state["radius"] == radius, k
        state.update(x_cost=dcost if valid else rec[k - 1][5], x_norm=0.0)
        if reason == 6:      # the tolerance that ended the solve is tested apart
            break
        out, _ = call(lm_shim, "step", state, opt, step_args(0.0, model, norm, why=0 if valid else STEP_INVALID_FACTORIZATION, new_cost=cost))
        state = dict(zip(STATE, out[1:1 + len(STATE)]))
        got = out[1 + len(STATE):8 + len(STATE)]
        assert (got[0], got[1], got[2]) == (valid, successful, reason), k
        if valid:
            assert got[6] == rho, k


def test_the_solve_loop_takes_the_controllers_decisions(shim, lm_shim):
    opt = {k: LM_OPT[k] for k in LM_OPT}
    # an honest quadratic: every step accepted with rho = 1 to rounding, the radius triples
    rc, t, rec, meta, msg = scripted(shim, 12, 1)
    assert rc == 0 and meta[1] == CONVERGENCE and msg == "Gradient tolerance reached."
    assert all(r[0] == 1 and r[1] == 1 for r in rec) and all(abs(r[4] - 1.0) <= 1e-9 for r in rec[1:])
    assert all(rec[k + 1][3] == rec[k][3] / (1.0 / 3.0) for k in range(1, len(rec) - 1))
    assert np.abs(t[:3] - 1.0).max() <= 1e-9 and np.abs(np.diff(t.reshape(-1, 3), axis=0) - [[0.5 + 0.25 * ((3 * i + k) % 5) for k in range(3)] for i in range(11)]).max() <= 1e-9
    replay(lm_shim, rec, opt)
    plain_cost = rec[-1][5]
    # the second candidate is reported far above the present cost: a rejected step, radius / 2, then the solve goes on
    rc, _, rec, meta, msg = scripted(shim, 12, 0, inflate=1)
    assert rc == 0 and meta[1] == CONVERGENCE
    assert (rec[2][0], rec[2][1], rec[2][2]) == (1, 0, STEP_REJECTED_RHO) and rec[3][3] == rec[2][3] / 2.0 and rec[2][5] == rec[1][5]
    replay(lm_shim, rec, opt)
    # the second linearisation has a negative diagonal entry: an invalid step, radius / 2, the point is linearised again and the solve goes on
    rc, _, rec, meta, msg = scripted(shim, 12, 1, bad_lin=1)
    assert rc == 0 and meta[1] == CONVERGENCE
    assert (rec[2][0], rec[2][1], rec[2][2]) == (0, 0, STEP_INVALID_FACTORIZATION) and rec[3][3] == 0.5 * rec[2][3] and rec[3][0] == 1
    replay(lm_shim, rec, opt)
    print("SPARSELM controller: %d records after an invalid step, final cost %.3e (undisturbed %.3e)" % (len(rec), rec[-1][5], plain_cost))
    # a callback fails: its code comes back, the arrays are untouched
    rc, t, rec, meta, _ = scripted(shim, 12, 0, fail_eval=4)
    assert rc == lc.ERR_HIP and np.all(t == 0.25)
    # the iteration limit
    rc, _, rec, meta, msg = scripted(shim, 12, 0, max_num_iterations=2)
    assert rc == 0 and meta[1] == 1 and meta[2] == 2 and msg == "Maximum number of iterations reached."


# ---- 6. sanitizers
def test_the_stand_alone_program_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "sparse_lm_host_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DSLH_MAIN"] + lc.INCLUDES + ["-o", exe, lc.SRC])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-2000:] + out.stderr[-2000:]


# ---- 7. exports
def test_the_library_builds_and_exports_the_new_entry_points():
    from solve_keyframe_pose_graph_amd import sparse_cholesky as sc
    lib = sc.load()
    txt = open(os.path.join(ROOT, "include", "pgo_sparse.h")).read()
    names = [n for n in _build.SPARSE_EXPORTS if n.startswith("pgo_sparse_lm_")]
    assert set(names) >= {"pgo_sparse_lm_create", "pgo_sparse_lm_destroy", "pgo_sparse_lm_set_scale", "pgo_sparse_lm_step", "pgo_sparse_lm_solve"}
    for name in names:
        assert hasattr(lib, name) and (" %s(" % name) in txt, name
    declared = {w.split("(")[0] for w in txt.replace("*", " ").split() if w.startswith("pgo_sparse_lm_") and "(" in w}
    assert declared == set(names)
    assert "pgo_sparse_lm.hpp" in _build.SPARSE_HEADERS and "pgo_sparse_lm_math.hpp" in _build.SPARSE_HEADERS and not {"pgo_sparse_lm.hpp", "pgo_sparse_lm_math.hpp"} & set(_build.HIP_HEADERS)
