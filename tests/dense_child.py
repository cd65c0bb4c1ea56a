"""Helper of tests/test_gpu_dense_cholesky.py, run as `python -m tests.dense_child` in a process of its own (the debug hooks' master switch is read once per process): C1
with the dense Cholesky solver, PGO_DEBUG_BREAK_DENSE=1 around the FIRST lm_step only, then the solve to its end; and the same solve undisturbed.  Prints ONE line
`DENSE <json>`: the first steps' records of the disturbed solve and both final costs (hex floats)."""
import json
import os

from solve_keyframe_pose_graph_amd import capi, graphgen
from tests import util


def solve(disturb):
    g = graphgen.config("C1")
    q, t, s = util.initial_state(g, True)
    P = util.pgo_problem(g, True, linear_solver=capi.LINEAR_DENSE_CHOLESKY, max_num_iterations=100, function_tolerance=1e-10)      # (both solves run to convergence)
    P.solve_begin(q, t, s)
    if disturb:
        os.environ["PGO_DEBUG_BREAK_DENSE"] = "1"
    try:
        done = P.lm_step()
    finally:
        os.environ.pop("PGO_DEBUG_BREAK_DENSE", None)
    while not done:
        done = P.lm_step()
    _, _, _, sm = P.solve_end()
    P.close()
    return sm


if __name__ == "__main__":
    broken, plain = solve(True), solve(False)
    rec = lambda it: dict(valid=int(it.step_is_valid), successful=int(it.step_is_successful), reason=int(it.reason), radius=float(it.trust_region_radius).hex(),
                          preconditioner=int(it.preconditioner), cg_iterations=int(it.cg_iterations))
    print("DENSE " + json.dumps(dict(steps=[rec(broken.iterations[k]) for k in range(min(broken.num_logged, 4))], unsuccessful=int(broken.num_unsuccessful_steps),
                                     termination=int(broken.termination_type), final_cost=float(broken.final_cost).hex(), plain_final_cost=float(plain.final_cost).hex(),
                                     plain_first_valid=int(plain.iterations[1].step_is_valid))))
