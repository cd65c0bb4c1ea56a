"""Helper of tests/test_gpu_param_covariance.py, run as `python -m tests.param_cov_child` in a process of its own (the debug hooks' master switch is read once per process):
pgo_covariance on the 24-keyframe graph with PGO_DEBUG_BREAK_DENSE=1 around the FIRST call only, then the same call again.  Prints ONE line `PARAMCOV <json>`: the first
call's error code, whether the output array was left alone, and whether the second call returned what an undisturbed handle returns."""
import ctypes as C
import json
import os

import numpy as np

from solve_keyframe_pose_graph_amd import capi
from tests import param_cov_ref as pref
from tests import precond_cases as pc
from tests import util

if __name__ == "__main__":
    g = pref.with_loops(24, [(10, 11), (23, 0), (5, 15)])
    q, t, s = pc.state(g)
    N = g.n_poses
    pairs = [(0, 0), (N + 0, N + 0), (3, N + 1), (N + 2, 17), (N + 1, N + 2)]
    P = util.pgo_problem(g, True)      # the default: matrix-free
    a = np.array([p[0] for p in pairs], np.int32); b = np.array([p[1] for p in pairs], np.int32)
    out = np.full((len(pairs), 36), 7.0)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    qq, tt, ss = P._state(q, t, s)
    os.environ["PGO_DEBUG_BREAK_DENSE"] = "1"
    try:
        rc = P.lib.pgo_covariance(P.h, qq.ctypes.data_as(dp), tt.ctypes.data_as(dp), ss.ctypes.data_as(dp), C.c_int64(N), C.c_int64(ss.size),
                                  C.c_int64(len(pairs)), a.ctypes.data_as(ip), b.ctypes.data_as(ip), out.ctypes.data_as(dp))
    finally:
        os.environ.pop("PGO_DEBUG_BREAK_DENSE", None)
    untouched = bool(np.all(out == 7.0))
    second = P.covariance(q, t, s, pairs)
    P.close()
    F = util.pgo_problem(g, True)
    fresh = F.covariance(q, t, s, pairs)
    F.close()
    same = all(np.array_equal(x, y) for x, y in zip(second, fresh))
    print("PARAMCOV " + json.dumps(dict(first_rc=int(rc), untouched=untouched, second_equals_fresh=bool(same), finite=bool(all(np.isfinite(x).all() for x in second)))))
