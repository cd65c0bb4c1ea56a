"""Helper of tests/test_gpu_precond_operator.py: the iterate of a k-step PCG of the first LM system of one of tests/precond_cases.py's graphs, through the C-ABI.
In process (linear_iterate) or, as `python -m tests.precond_child '<json>'`, in a process of its own — the debug hooks of csrc/pgo_handle.hpp are read once per process —
printing ONE line `ITERATE <json>` with the iterate as hex floats, the step's iteration record and whether the PCG captured a chunk."""
import json
import sys

import numpy as np


def linear_iterate(graph, k, radius, constant=(), drop_last=0, handle=None, regroup=None, **opt):
    """-> (x [6 N], pgo_iteration of the step, the handle).  One handle serves several k: cg_max_iterations is set per solve.  regroup: the start values are
    precond_cases.state(g, regroup) — a solve from "B" on a handle that last solved from "A" starts with a regroup."""
    from tests import precond_cases as pc
    from tests import util
    g = pc.graph(graph, drop_last)
    q, t, s = pc.state(g, regroup)
    base = dict(cg_early_tolerance=0.0, cg_mid_tolerance=0.0, mg_switch_iterations=0, initial_trust_region_radius=radius, cg_max_iterations=k)
    base.update(opt)
    if handle is None:
        handle = util.pgo_problem(g, True, **base)
        if constant:
            handle.set_nodes_constant(list(constant))
    else:
        handle.set_options(**base)
    handle.solve_begin(q, t, s)
    handle.lm_step()
    x = handle.linear_solution()
    _, _, _, sm = handle.solve_end()
    return x, sm.iterations[1], handle


if __name__ == "__main__":
    a = json.loads(sys.argv[1])
    x, it, P = linear_iterate(a["graph"], a["k"], a["radius"], tuple(a.get("constant", ())), a.get("drop_last", 0), **a.get("opt", {}))
    P.close()
    print("ITERATE " + json.dumps({"x": [float(v).hex() for v in x], "cg_iterations": int(it.cg_iterations), "preconditioner": int(it.preconditioner), "single_reduction": int(it.single_reduction)}))
