"""GPU: the split single-reduction update of the multigrid PCG gives the bits of the unsplit one.

With the restriction inside the vector update (one GPU, single-reduction form) the update is split: cg_update_mg_crit_kernel does what the cycle waits for, the rest
(p, x, the block-Jacobi part of the next u, the partials of r.u) rides as extra workgroups in two of the cycle's sparse-level launches.  No sum changes its order, so
the criterion is equality: every graph below is solved in SEPARATE processes with the split and with PGO_DEBUG_NO_SPLIT_UPDATE=1 (the unsplit cg_update_mg_kernel<true>),
with library defaults, under PGO_DEBUG_POISON=1 and with cg_use_graph=0 — all six digests (every output array, the whole iteration log) must be the same.
  deep_rejected   12 000 keyframes, switchable loop closures, hierarchy of four levels: its solve has rejected steps, pauses and resumes
  deep_plain      9 000 keyframes, plain loops, chain-like, four levels
  shallow         6 000 keyframes, plain loops, the default dense level: level 2 (<= 512 nodes) is already the dense one, so fewer than two launches could carry a
                  rider and the unsplit kernel runs BY RULE, hook or no hook
  explicit        640 keyframes (tests/precond_cases.py's multigrid graph), three levels, level 1 with an explicit transfer operator: its down-sweep is mg_sdown_kernel, and
                  the eligible launches are that one and level 2's two (level 1's up-sweep is the fused one)
  explicit_deep   the same graph with level 2 smoothed as well: the rule's pair is level 2's mg_sdown_kernel launch and its up-sweep, which reads the dense level's solution
                  itself (xn) — riders carried by an explicit-transfer level
Which path the HOST chose is read off pgo_time_kernel(6)'s byte count (the split iteration reads the residual once more, 48 B per keyframe): it witnesses the rule's decision
only — that the riders then ran is what the digests show, since a rider that did not run leaves x, p and z stale.
PGO_DEBUG_SPLIT_HOSTS (the scan hook behind DESIGN.md §9's host variants) is held to the same bits: both riders in ONE launch, and a pair other than the rule's.

Run as `python -m tests.test_gpu_split_update <graph> [opt=value ...]` this file is its own helper: one solve, one DIGEST line."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.precond_cases import MG_BASE

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the smoothed keyframe transition off: the restriction then rides in the vector update (MgDev::blk_tab); 64 dense nodes: two sparse levels more than the default's 512
GRAPHS = {
    "deep_rejected": (dict(n=12000, loops=12000, odom_f_max=2, seed=3), True, dict(mg_smoothed_fine=0, mg_dense_max_nodes=64)),
    "deep_plain": (dict(n=9000, loops=900, odom_f_max=1, seed=2, outlier_frac=0.0), False, dict(mg_smoothed_fine=0, mg_dense_max_nodes=64)),
    "shallow": (dict(n=6000, loops=600, odom_f_max=1, seed=2, outlier_frac=0.0), False, dict(mg_smoothed_fine=0)),
    "explicit": ("mg640", True, dict(MG_BASE, mg_smoothed_levels=1, mg_explicit_transfer=1, mg_passes=2, mg_dense_max_nodes=16)),
    "explicit_deep": ("mg640", True, dict(MG_BASE, mg_smoothed_levels=2, mg_explicit_transfer=1, mg_passes=2, mg_dense_max_nodes=16)),
}


def digest(name, **opt):
    from solve_keyframe_pose_graph_amd import capi, graphgen
    from tests import util
    spec, switchable, base = GRAPHS[name]
    if isinstance(spec, str):
        from tests import precond_cases
        g = precond_cases.graph(spec)
    else:
        spec = dict(spec)
        g = graphgen.generate(spec.pop("n"), spec.pop("loops"), **spec)
    q, t, s = util.initial_state(g, switchable)
    kw = dict(base); kw.update(opt)
    P = util.pgo_problem(g, switchable, **kw)
    qo, to, so, sm = P.solve(q, t, s)
    P.solve_begin(q, t, s)
    _, iteration_bytes = P.time_kernel(6, 2)
    P.solve_end()
    P.close()
    h = hashlib.sha256(np.ascontiguousarray(qo).tobytes() + np.ascontiguousarray(to).tobytes() + np.ascontiguousarray(so).tobytes()).hexdigest()
    log = [[it.iteration, it.step_is_valid, it.step_is_successful, capi.STEP_REASONS[it.reason], it.preconditioner, it.cg_iterations, float(it.cost).hex(), float(it.relative_decrease).hex()]
           for it in (sm.iterations[k] for k in range(sm.num_logged))]
    return {"graph": name, "keyframes": int(np.asarray(t).size // 3), "sha256": h, "final_cost": float(sm.final_cost).hex(),
            "cg_iterations": int(sm.cg_iterations), "cg_iterations_multigrid": int(sm.cg_iterations_multigrid), "iteration_bytes": int(iteration_bytes), "log": log}


def digest_in_a_new_process(name, split, poison=False, hosts=None, **opt):
    env = dict(os.environ)
    env["PGO_ENABLE_DEBUG_HOOKS"] = "1"      # (the hooks need the master switch: csrc/pgo_handle.hpp)
    for k in ("PGO_DEBUG_POISON", "PGO_DEBUG_NO_SPLIT_UPDATE", "PGO_DEBUG_SPLIT_HOSTS", "PGO_LIBPGO_OVERRIDE"):
        env.pop(k, None)
    if poison:
        env["PGO_DEBUG_POISON"] = "1"
    if not split:
        env["PGO_DEBUG_NO_SPLIT_UPDATE"] = "1"
    if hosts:
        env["PGO_DEBUG_SPLIT_HOSTS"] = hosts
    cmd = [sys.executable, "-m", "tests.test_gpu_split_update", name] + ["%s=%r" % kv for kv in opt.items()]
    out = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("DIGEST ")][-1]
    return json.loads(line[len("DIGEST "):])


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_split_and_unsplit_update_give_the_same_bits(name):
    runs = {}
    for label, kw in (("defaults", {}), ("poisoned", dict(poison=True)), ("no graph", dict(cg_use_graph=0))):
        for split in (True, False):
            runs[(label, split)] = digest_in_a_new_process(name, split, **kw)
    ref = runs[("defaults", False)]
    print(name, {k: (v["sha256"][:12], v["cg_iterations"], v["cg_iterations_multigrid"], v["iteration_bytes"]) for k, v in runs.items()})
    assert ref["cg_iterations_multigrid"] > 0, "the multigrid never ran: the graph does not exercise the update under test"
    for key, d in runs.items():
        assert d["log"] == ref["log"], (key, d["log"], ref["log"])
        assert d["sha256"] == ref["sha256"] and d["final_cost"] == ref["final_cost"] and d["cg_iterations"] == ref["cg_iterations"], key
    # which update ran: the split iteration reads r once more, 48 B per keyframe
    extra = runs[("defaults", True)]["iteration_bytes"] - ref["iteration_bytes"]
    assert extra == (0 if name == "shallow" else 48 * ref["keyframes"]), (extra, ref["keyframes"])
    if name == "deep_rejected":
        assert any(rec[2] == 0 for rec in ref["log"]), "no rejected step: the graph no longer exercises pauses and resumes"


def hosts_give_the_same_bits(name, hosts):
    ref = digest_in_a_new_process(name, False)
    d = digest_in_a_new_process(name, True, hosts=hosts)
    assert d["iteration_bytes"] - ref["iteration_bytes"] == 48 * ref["keyframes"]
    assert d["log"] == ref["log"], (d["log"], ref["log"])
    assert d["sha256"] == ref["sha256"] and d["final_cost"] == ref["final_cost"] and d["cg_iterations"] == ref["cg_iterations"]


@pytest.mark.parametrize("hosts", ["0,0", "0,1", "1,1"])
def test_other_host_launches_give_the_same_bits(hosts):
    """Eligible launches of deep_rejected's cycle come in launch order, the down-sweeps first.  "0,0" / "1,1": one launch carries both riders (a lane rewrites the z
    entries it has read itself); "0,1": the level-1 and level-2 down-sweeps, not the rule's pair."""
    hosts_give_the_same_bits("deep_rejected", hosts)


def test_an_explicit_transfer_down_sweep_as_host_gives_the_same_bits():
    """`explicit`'s first eligible launch is level 1's mg_sdown_kernel launch — the one with the most workgroups of its own, which the rule never picks: here it carries the
    direction / solution rider, level 2's down-sweep the block-Jacobi one."""
    hosts_give_the_same_bits("explicit", "0,1")


if __name__ == "__main__":
    kw = {}
    for a in sys.argv[2:]:
        k, v = a.split("=")
        kw[k] = float(v) if ("." in v or "e" in v) else int(v)
    print("DIGEST " + json.dumps(digest(sys.argv[1], **kw)))
