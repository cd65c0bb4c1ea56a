"""Helper of tests/test_gpu_dense_covariance.py, run as `python -m tests.dense_cov_child` in a process of its own (the debug hooks' master switch is read once per process):
pgo_pose_covariance on the 22-keyframe graph with PGO_DEBUG_BREAK_DENSE=1 around the FIRST call only, then the same call again.  Prints ONE line `DENSECOV <json>`: the
first call's error code, whether the output array was left alone, and whether the second call returned what an undisturbed handle returns."""
import ctypes as C
import json
import os

import numpy as np

from solve_keyframe_pose_graph_amd import capi
from tests import precond_cases as pc
from tests import util

if __name__ == "__main__":
    g = util.small_graph(22, 3, f=3, seed=11)
    q, t, s = pc.state(g)
    pairs = [(0, 0), (21, 21), (3, 17)]
    P = util.pgo_problem(g, True, linear_solver=capi.LINEAR_PCG_BLOCK_JACOBI)
    a = np.array([p[0] for p in pairs], np.int32); b = np.array([p[1] for p in pairs], np.int32)
    out = np.full((len(pairs), 6, 6), 7.0)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    qq, tt, ss = P._state(q, t, s)
    os.environ["PGO_DEBUG_BREAK_DENSE"] = "1"
    try:
        rc = P.lib.pgo_pose_covariance(P.h, qq.ctypes.data_as(dp), tt.ctypes.data_as(dp), ss.ctypes.data_as(dp) if ss.size else None, C.c_int64(g.n_poses), C.c_int64(ss.size),
                                       C.c_int64(len(pairs)), a.ctypes.data_as(ip), b.ctypes.data_as(ip), out.ctypes.data_as(dp))
    finally:
        os.environ.pop("PGO_DEBUG_BREAK_DENSE", None)
    untouched = bool(np.all(out == 7.0))
    second = P.pose_covariance(q, t, s, pairs)
    P.close()
    F = util.pgo_problem(g, True, linear_solver=capi.LINEAR_PCG_BLOCK_JACOBI)
    fresh = F.pose_covariance(q, t, s, pairs)
    F.close()
    print("DENSECOV " + json.dumps(dict(first_rc=int(rc), untouched=untouched, second_equals_fresh=bool(np.array_equal(second, fresh)), finite=bool(np.isfinite(second).all()))))
