"""The calls whose returned bits tests/golden/pcg_kernel_bits.json records: what scripts/record_pcg_kernel_bits.py (which writes the file) and
tests/test_gpu_pcg_bits.py (which compares against it) share.  The PCG iteration's kernels (csrc/pgo_kernels.hip, csrc/pgo_mg_kernels.hpp, their shared statements
in csrc/pgo_pcg_ops.hpp) through the iterate x_k of a k-step PCG of the first LM system (tests/precond_child.linear_iterate), at the smallest graphs the repository
uses for these forms (tests/precond_cases.GRAPHS: 300, 600 and 640 keyframes — aggregates of whole and partial size, a second workgroup trip, a hierarchy with two
sparse levels for the split update):

  "<label> @ <radius>"     every form of precond_cases.FORMS at both radii of precond_cases.RADII, k in precond_cases.KS on one handle: block-Jacobi classic,
                           single-reduction and block-CSR; the two-level method fused classic, fused single-reduction and unfused; the multigrid with the restricted
                           classic and single-reduction update, the split update and block-CSR;
  "two-level direct"       one aggregate per keyframe (tl200 with the default coarse_aggregates): the `direct` branches of cg_update_restrict_kernel and of
                           sr_head(..., coarse_only) run only there;
  "two-level constant"     CONSTANT_TL600 and three unreferenced keyframes at the end, fused: the free flag multiplies the rigid-mode transfer;
  "two-level converged"    cg_rel_tolerance = 1e-11 under a cap of 5 000: the stop rule's converged branch; x and the iteration count.

No case with several ranks: pgo_get_linear_solution refuses a handle with a communicator, so cgcg_update_kernel's iterate cannot be read the way the others are;
tests/test_gpu_two_ranks_one_gpu.py covers that kernel.

run(name) returns (inputs, outputs): a list of arrays (graph arrays, start state, the options as sorted text) and a dict of arrays; digests(name) their sha256
(tests/dense_bits_cases.sha)."""
import numpy as np

from tests import precond_cases as pc
from tests.dense_bits_cases import sha
from tests.precond_child import linear_iterate

# name -> (graph, constant, unreferenced at the end, options, radius, iteration counts, preconditioner expected)
CASES = {}
for _label in sorted(pc.FORMS):
    for _radius in pc.RADII:
        CASES["%s @ %.0e" % (_label, _radius)] = (pc.FORMS[_label][0], (), 0, pc.FORMS[_label][1], _radius, pc.KS, pc.FORMS[_label][2])
CASES["two-level direct"] = ("tl200", (), 0, dict(), pc.RADII[0], pc.KS, pc.TL)
CASES["two-level constant"] = ("tl600", pc.CONSTANT_TL600, 3, dict(coarse_aggregates=64), pc.RADII[0], pc.KS, pc.TL)
CASES["two-level converged"] = ("tl600", (), 0, dict(coarse_aggregates=64, cg_rel_tolerance=1e-11), pc.RADII[0], (5000,), pc.TL)
CASE_NAMES = tuple(sorted(CASES))


def inputs_of(name):
    graph, constant, drop, opt, radius, ks, _ = CASES[name]
    g = pc.graph(graph, drop)
    q, t, s = pc.state(g)
    text = repr(sorted(opt.items())) + " radius %r k %r constant %r" % (radius, tuple(ks), tuple(constant))
    return [g.odom_c1, g.odom_c2, g.odom_T, g.odom_w, g.loop_c1, g.loop_c2, g.loop_T, g.loop_w, g.reg_node, g.reg_T, g.reg_w, q, t, s, np.frombuffer(text.encode(), np.uint8)]


def run(name):
    graph, constant, drop, opt, radius, ks, precond = CASES[name]
    P, out = None, {}
    for k in ks:
        x, it, P = linear_iterate(graph, k, radius, constant, drop, handle=P, **opt)
        assert it.preconditioner == precond, (name, it.preconditioner)
        out["x_%d" % k] = x
        out["record_%d" % k] = np.array([it.cg_iterations, it.preconditioner, it.single_reduction], np.int64)
    P.close()
    return inputs_of(name), out


def digests(name):
    """{"inputs": sha256 of the input bytes, "outputs": {name: sha256 of that output's bytes}}"""
    inputs, outputs = run(name)
    return {"inputs": sha(inputs), "outputs": {k: sha([v]) for k, v in sorted(outputs.items())}}
