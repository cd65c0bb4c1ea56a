"""CPU: the dense fp64 model of the preconditioners (tests/precond_model.py) that tests/test_gpu_precond_operator.py compares the HIP kernels with — its own sanity, and
its TEETH: every deliberately wrong variant of a preconditioner (a post-smoothing step dropped on one level, omega = 1, the factor 2 of [d]x missing, the centroid
over all members instead of the free ones, a restriction without the cross term) differs from the model by more than 100 x the tolerance the GPU test grants the
device, 8 e_ref with e_ref = |M_32 - M_64| / |M_64| (max-norms) — so the GPU test would catch each of them.  The graphs and radii are the GPU test's own; the
multigrid aggregates come from the host hierarchy builder (tests/native/mg_host.cpp).

The cases of the smoother's safety rescaling, of the smoothed keyframe transition and of a hierarchy after a regroup (pc.MG_PATH_CASES, pc.MG_REGROUP_CASES) have their
conditions here — which sparse level is rescaled and which is not, each 0.01 clear of the limit; definiteness; the bound a bound; the regrouped hierarchy differs from the
first and equals a fresh build — and their own teeth: the limit never applied, applied to every level, Ps formed before the rescaling, the three ways the keyframe
transition can be half-smoothed, the previous hierarchy left in place."""
import functools

import numpy as np
import pytest

from tests import precond_cases as pc
from tests import precond_model as pm


def rel(X, ref):
    return pm.maxnorm(X) / pm.maxnorm(ref)


def is_positive_definite(M):
    try:
        np.linalg.cholesky(0.5 * (M + M.T))
        return True
    except np.linalg.LinAlgError:
        return False


@pytest.fixture(scope="module")
def two_level_models():
    """two-level method on the 600-keyframe graph with constant and unreferenced keyframes, both radii: (lin, A, b, m, M_64 model, M_32 model)"""
    out = {}
    lin = pc.linearisation("tl600", pc.CONSTANT_TL600, 3)
    m, _ = pm.two_level_aggregates(600, 64)
    for radius in pc.RADII:
        A, b = pc.system("tl600", radius, pc.CONSTANT_TL600, 3)
        out[radius] = (lin, A, b, m, pm.two_level(lin, A, m), pm.two_level(lin, A, m, fp32=True))
    return out


def mg_model(case, radius, constant=(), fp32=False, **kw):
    return _mg_model(case, radius, constant, fp32, tuple(sorted((k, tuple(sorted(v.items())) if isinstance(v, dict) else v) for k, v in kw.items())))


@functools.lru_cache(maxsize=None)
def _mg_model(case, radius, constant, fp32, kw_items):
    kw = {k: dict(v) if isinstance(v, tuple) else v for k, v in kw_items}
    _, margs, _ = pc.MG_CASES[case]
    lin = pc.linearisation("mg640", constant)
    g = pc.graph("mg640")
    _, _, s = pc.state(g)
    agg0, parents, sizes = pc.host_hierarchy(g, lin.free, s, margs["passes"], margs["dense_max"], margs["smoothed_levels"])
    A, b = pc.system("mg640", radius, constant)
    args = dict(smoothed_levels=margs["smoothed_levels"], explicit=margs["explicit"])
    args.update(kw)
    return lin, A, b, sizes, pm.multigrid(lin, A, agg0, parents, fp32=fp32, **args)


def test_aggregate_rule_gives_the_cases_the_gpu_test_names():
    assert pm.two_level_aggregates(200, 768) == (1, 200)       # one aggregate per keyframe
    assert pm.two_level_aggregates(600, 64) == (10, 60)
    assert pm.two_level_aggregates(601, 64) == (10, 61)        # a last aggregate of one keyframe
    assert pm.two_level_aggregates(600, 8) == (75, 8)          # > 64 keyframes: the unfused form
    assert pm.two_level_aggregates(300, 0) is None


def test_system_drops_constant_and_unreferenced_keyframes():
    lin = pc.linearisation("tl600", pc.CONSTANT_TL600, 3)
    assert not lin.free[list(pc.CONSTANT_TL600)].any() and not lin.free[597:].any() and lin.free.sum() == 600 - 15 - 3
    A, b = pc.system("tl600", 1e4, pc.CONSTANT_TL600, 3)
    assert A.shape == (6 * 582, 6 * 582) and is_positive_definite(A)


@pytest.mark.parametrize("radius", pc.RADII)
def test_two_level_model_sanity(two_level_models, radius):
    lin, A, b, m, m64, m32 = two_level_models[radius]
    M, Cc, P = m64["M"], m64["C"], m64["P"]
    assert P.shape[1] == 6 * 59                                  # 60 aggregates, one of them without a free keyframe
    assert rel(M - M.T, M) <= 1e-12
    assert is_positive_definite(M) and is_positive_definite(m32["M"])      # ... the fp32 Ac^-1 too, at the largest radius used
    # the coarse correction is the A-orthogonal projector onto the aggregates' rigid motions
    assert rel(Cc @ A @ Cc - Cc, Cc) <= 1e-7
    assert rel(Cc @ (A @ P) - P, P) <= 1e-7
    if radius == pc.RADII[0]:
        assert pm.pcg_iterations(A, b, M, 1e-6) < pm.pcg_iterations(A, b, pm.block_jacobi(A), 1e-6)
    assert 8 * rel(m32["M"] - M, M) <= 1e-3


def test_two_level_one_aggregate_per_keyframe_is_the_inverse():
    lin = pc.linearisation("tl200")
    for radius in pc.RADII:
        A, _ = pc.system("tl200", radius)
        m64, m32 = pm.two_level(lin, A, 1), pm.two_level(lin, A, 1, fp32=True)
        assert rel(m64["M"] @ A - np.eye(len(A)), np.eye(1)) <= 1e-8
        assert is_positive_definite(m32["M"]) and 8 * rel(m32["M"] - m64["M"], m64["M"]) <= 1e-3


@pytest.mark.parametrize("radius", pc.RADII)
@pytest.mark.parametrize("case", sorted(pc.MG_CASES))
def test_multigrid_model_sanity(case, radius):
    lin, A, b, sizes, m64 = mg_model(case, radius)
    _, _, _, _, m32 = mg_model(case, radius, fp32=True)
    M = m64["M"]
    assert len(sizes) == pc.MG_CASES[case][2] == m64["n_levels"]
    assert rel(M - M.T, M) <= 1e-12
    assert is_positive_definite(M) and is_positive_definite(m32["M"])
    # the smoother limit is clear of its threshold on this graph (precond_cases.py): no rescaling, in the model and on the device alike
    assert not m64["limit_active"] and not m32["limit_active"]
    assert pc.limit_margin(m64) >= 0.01 and pc.limit_margin(m32) >= 0.01
    assert all(pm.OMEGA * lam < 2.0 for lam in m64["lam_max"])
    # the cycle is a convergent symmetric iteration: the eigenvalues of (M^-1 - D^-1) A / s = P_0 V P_0^T A lie in [0, 1] — the nonzero ones are those of V A_1 (s = 1)
    L1 = np.linalg.cholesky(m64["A1"])
    ev = np.linalg.eigvalsh(L1.T @ m64["V"] @ L1)
    assert ev[0] > 0.0 and ev[-1] <= 1.0 + 1e-9
    assert 8 * rel(m32["M"] - M, M) <= 1e-3


@pytest.mark.parametrize("case", ["one_sparse", "smoothed_expl"])
def test_multigrid_model_saves_pcg_iterations(case):
    lin, A, b, sizes, m64 = mg_model(case, 1e7)
    assert pm.pcg_iterations(A, b, m64["M"], 1e-6) < pm.pcg_iterations(A, b, pm.block_jacobi(A), 1e-6)


def test_implicit_and_explicit_smoothed_transition_are_the_same_operator():
    _, _, _, _, a = mg_model("smoothed_impl", 1e4)
    _, _, _, _, b = mg_model("smoothed_expl", 1e4)
    assert rel(a["M"] - b["M"], a["M"]) <= 1e-12


def test_multigrid_with_constant_keyframes_leaves_them_out():
    lin, A, b, sizes, m64 = mg_model("one_sparse", 1e4, constant=pc.CONSTANT_MG640)
    assert len(A) == 6 * (640 - 30) and is_positive_definite(m64["M"]) and not m64["limit_active"] and pc.limit_margin(m64) >= 0.01


# ---- the paths the library takes by default on real graphs (pc.MG_PATH_CASES, pc.MG_REGROUP_CASES): what the GPU tests of these cases may rely on ----
@functools.lru_cache(maxsize=None)
def path_hierarchy(case):
    graph, _, margs, _, _ = pc.MG_PATH_CASES[case]
    g, lin = pc.graph(graph), pc.linearisation(graph)
    _, _, s = pc.state(g)
    return pc.host_hierarchy(g, lin.free, s, margs["passes"], margs["dense_max"], margs["smoothed_levels"], fine=margs.get("smoothed_fine", False))


def path_model(case, radius, fp32=False, variant=None):
    """variant: the NAME of one of precond_model.multigrid's wrong devices (not kept: each is looked at once)"""
    if variant is None:
        return _path_model(case, radius, fp32)
    graph, _, margs, _, _ = pc.MG_PATH_CASES[case]
    agg0, parents, _ = path_hierarchy(case)
    A, _ = pc.system(graph, radius)
    return pm.multigrid(pc.linearisation(graph), A, agg0, parents, fp32=fp32, variant={variant: True}, **pc.model_arguments(margs))


@functools.lru_cache(maxsize=None)
def _path_model(case, radius, fp32):
    graph, _, margs, _, _ = pc.MG_PATH_CASES[case]
    agg0, parents, _ = path_hierarchy(case)
    A, _ = pc.system(graph, radius)
    m = pm.multigrid(pc.linearisation(graph), A, agg0, parents, fp32=fp32, **pc.model_arguments(margs))
    del m["C"], m["levels"]      # (kept for the teeth tests below: M and the small pieces only)
    return m


@functools.lru_cache(maxsize=None)
def regroup_hierarchies(case):
    """(the hierarchy of state A, the one a regroup from A's cache gives at state B, the fresh build from B's switches)"""
    _, margs, _ = pc.MG_REGROUP_CASES[case]
    g, lin = pc.graph("mg640"), pc.linearisation("mg640")
    (_, _, sa), (_, _, sb) = pc.state(g), pc.state(g, "B")
    shape = (margs["passes"], margs["dense_max"], margs["smoothed_levels"])
    return pc.host_hierarchy(g, lin.free, sa, *shape), pc.host_hierarchy(g, lin.free, sb, *shape, s_first=sa), pc.host_hierarchy(g, lin.free, sb, *shape)


def same_hierarchy(a, b):
    return np.array_equal(a[0], b[0]) and len(a[1]) == len(b[1]) and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))


def check_path_conditions(m64, m32, rescaled):
    """the conditions under which the GPU test's comparison means something: both models symmetric positive definite, the bound a bound, every sparse level on the side of
    the smoother limit the case names and clear of it by 0.01 — level by level —, the cycle a convergent symmetric iteration"""
    M = m64["M"]
    assert rel(M - M.T, M) <= 1e-12 and rel(m32["M"] - m32["M"].T, M) <= 1e-12
    assert is_positive_definite(M) and is_positive_definite(m32["M"])
    assert 8 * rel(m32["M"] - M, M) <= 1e-3
    for m in (m64, m32):
        assert m["rescaled"] == list(rescaled) and m["limit_active"] == any(rescaled), (m["rescaled"], m["lam_est"])
        assert all(pc.limit_margin(dict(lam_est=[e])) >= 0.01 for e in m["lam_est"]), m["lam_est"]
    # with the weight the smoother ends up with (a rescaled level: omega lambda_est = 1.5) every level's omega lambda_max stays below 2 ...
    for lam, est, on in zip(m64["lam_max"], m64["lam_est"], m64["rescaled"]):
        assert (pm.SMOOTHER_TARGET / est if on else pm.OMEGA) * lam < 2.0
    # ... and the cycle is a convergent symmetric iteration on level 1: the eigenvalues of V A_1 lie in (0, 1]
    L1 = np.linalg.cholesky(m64["A1"])
    ev = np.linalg.eigvalsh(L1.T @ m64["V"] @ L1)
    assert ev[0] > 0.0 and ev[-1] <= 1.0 + 1e-9


@pytest.mark.parametrize("radius", pc.RADII)
@pytest.mark.parametrize("case", sorted(pc.MG_PATH_CASES))
def test_path_model_conditions(case, radius):
    _, _, _, n_levels, rescaled = pc.MG_PATH_CASES[case]
    m64, m32 = path_model(case, radius), path_model(case, radius, fp32=True)
    assert len(path_hierarchy(case)[2]) == n_levels == m64["n_levels"]
    check_path_conditions(m64, m32, rescaled)


def test_rescaled_implicit_and_explicit_are_the_same_operator():
    a, b = path_model("rescaled_smoothed_impl", 1e4), path_model("rescaled_smoothed_expl", 1e4)
    assert rel(a["M"] - b["M"], a["M"]) <= 1e-12


@pytest.mark.parametrize("radius", pc.RADII)
def test_without_the_rescaling_the_cycle_is_not_positive_definite(radius):
    """what the branch is for: level 1 of fine_rescaled has omega lambda_max = 2.25, and the unrescaled smoother makes M^-1 indefinite"""
    assert path_model("fine_rescaled", radius)["lam_max"][0] * pm.OMEGA > 2.0
    assert not is_positive_definite(path_model("fine_rescaled", radius, variant="no_rescale")["M"])


@pytest.mark.parametrize("radius", pc.RADII)
@pytest.mark.parametrize("case", sorted(pc.MG_REGROUP_CASES))
def test_regroup_model_conditions(case, radius):
    _, margs, n_levels = pc.MG_REGROUP_CASES[case]
    at_a, regrouped, fresh = regroup_hierarchies(case)
    assert not same_hierarchy(at_a, regrouped)                           # the regroup does move aggregates ...
    assert same_hierarchy(regrouped, fresh)                              # ... to where a fresh build from B's switches puts them
    assert len(regrouped[2]) == n_levels
    lin = pc.linearisation("mg640", regroup="B")
    A, _ = pc.system("mg640", radius, regroup="B")
    kw = pc.model_arguments(margs)
    m64, m32 = pm.multigrid(lin, A, regrouped[0], regrouped[1], **kw), pm.multigrid(lin, A, regrouped[0], regrouped[1], fp32=True, **kw)
    check_path_conditions(m64, m32, (False,) * (n_levels - 1))
    # teeth: the hierarchy of state A left in place at B's system
    tol = 8 * rel(m32["M"] - m64["M"], m64["M"]) + 1e-10
    stale = pm.multigrid(lin, A, at_a[0], at_a[1], **kw)
    assert rel(stale["M"] - m64["M"], m64["M"]) > 100 * tol


def test_reference_pcg_converges_to_the_solution():
    lin = pc.linearisation("tl200")
    A, b = pc.system("tl200", 1e4)
    xs = pm.pcg(A, b, pm.two_level(lin, A, 10)["M"], 120)
    x = np.linalg.solve(A, b)
    assert pm.maxnorm(xs[-1] - x) <= 1e-9 * pm.maxnorm(x) and pm.maxnorm(xs[0] - x) > 1e-3 * pm.maxnorm(x)


# ---- teeth ----
@pytest.mark.parametrize("radius", pc.RADII)
def test_centroid_choice_alone_does_not_change_the_two_level_operator(two_level_models, radius):
    """Moving an aggregate's centroid (over all members instead of the free ones) multiplies P by an invertible block-diagonal matrix from the right: the coarse SPACE and
    with it P (P^T A P)^-1 P^T stay the same, so no operator test can see that choice as long as the coarse operator and the transfers use the same centroids.  What a
    test can see — and test_teeth_two_level[centroid_all] shows it does — is the coarse operator assembled with one centroid and the transfers applied with the other."""
    lin, A, b, m, m64, m32 = two_level_models[radius]
    same = pm.two_level(lin, A, m, variant=dict(centroid_all=True))
    assert rel(same["d"] - m64["d"], m64["d"]) > 1e-3                    # the offsets do differ (aggregates 2 and 4 have constant members)
    assert rel(same["M"] - m64["M"], m64["M"]) <= 1e-9


@pytest.mark.parametrize("radius", pc.RADII)
@pytest.mark.parametrize("variant", [dict(factor=1.0), dict(transfer_centroid_all=True), dict(restrict_no_cross=True)], ids=["factor2", "centroid_all", "restrict_no_cross"])
def test_teeth_two_level(two_level_models, variant, radius):
    lin, A, b, m, m64, m32 = two_level_models[radius]
    tol = 8 * rel(m32["M"] - m64["M"], m64["M"]) + 1e-10
    wrong = pm.two_level(lin, A, m, variant=variant)
    assert rel(wrong["M"] - m64["M"], m64["M"]) > 100 * tol


@pytest.mark.parametrize("radius", pc.RADII)
@pytest.mark.parametrize("case,kw", [("three_levels", dict(variant=dict(drop_post_level=1))), ("three_levels", dict(variant=dict(drop_post_level=2))), ("smoothed_expl", dict(omega=1.0)),
                                     ("one_sparse", dict(omega=1.0)), ("one_sparse", dict(variant=dict(factor=1.0))), ("dense", dict(variant=dict(restrict_no_cross=True))),
                                     ("smoothed_impl", dict(variant=dict(drop_post_level=1)))],
                         ids=["drop_post_1", "drop_post_2", "omega_smoothed", "omega", "factor2", "restrict_no_cross", "drop_post_smoothed"])
def test_teeth_multigrid(case, kw, radius):
    _, _, _, _, m64 = mg_model(case, radius)
    _, _, _, _, m32 = mg_model(case, radius, fp32=True)
    tol = 8 * rel(m32["M"] - m64["M"], m64["M"]) + 1e-10
    _, _, _, _, wrong = mg_model(case, radius, **kw)
    assert rel(wrong["M"] - m64["M"], m64["M"]) > 100 * tol


# every plausibly wrong device of the rescaling and of the smoothed keyframe transition, on each case it can show on: (case, variant of precond_model.multigrid)
PATH_TEETH = [("rescaled_plain", "no_rescale"), ("rescaled_smoothed_impl", "no_rescale"), ("rescaled_smoothed_expl", "no_rescale"), ("fine_rescaled", "no_rescale"),
              ("rescaled_plain", "rescale_every_level"), ("fine_rescaled", "rescale_every_level"),
              ("fine_rescaled", "ps_before_rescale"),      # (the rescaled level of the rescaled_* cases has no smoothed transition above it: nothing to see there)
              ("fine640", "fine_restrict_plain"), ("fine640", "fine_level1_plain"), ("fine640", "fine_omega_p")]


@pytest.mark.parametrize("radius", pc.RADII)
@pytest.mark.parametrize("case,variant", PATH_TEETH, ids=["%s-%s" % cv for cv in PATH_TEETH])
def test_teeth_paths(case, variant, radius):
    m64, m32 = path_model(case, radius), path_model(case, radius, fp32=True)
    tol = 8 * rel(m32["M"] - m64["M"], m64["M"]) + 1e-10
    wrong = path_model(case, radius, variant=variant)
    assert rel(wrong["M"] - m64["M"], m64["M"]) > 100 * tol
