// Test-only host instantiation of the yaw/pitch/roll-weighted edge of csrc/pgo_device_math.hpp (relpose_residual_ypr, relpose_residual_ypr_robust: the
// per-edge evaluation; the YPR forms of compact_apply / compact_apply_both: the matrix-free product) so that they can be checked against tests/golden without a GPU.
// Not a product path.  The observation goes in as the edge record holds it (quaternion and translation), so that both signs of the quaternion can be given.
#include "pgo_device_math.hpp"
using namespace pgo;
extern "C" {
static Pose mk(const double* q, const double* t) { return Pose{q[0], q[1], q[2], q[3], t[0], t[1], t[2]}; }
static Meas mkm(const double* qo, const double* to, double w) { return Meas{qo[0], qo[1], qo[2], qo[3], to[0], to[1], to[2], w}; }
void yh_relpose(const double* q1, const double* t1, const double* q2, const double* t2, const double* qo, const double* to, double w, const double* g3, double* r, double* J1, double* J2) {
    relpose_residual_ypr<true>(mk(q1, t1), mk(q2, t2), mkm(qo, to, w), w, g3, r, J1, J2);
}
void yh_relpose_cost_only(const double* q1, const double* t1, const double* q2, const double* t2, const double* qo, const double* to, double w, const double* g3, double* r) {
    relpose_residual_ypr<false>(mk(q1, t1), mk(q2, t2), mkm(qo, to, w), w, g3, r, nullptr, nullptr);
}
// enc: +a Huber(a), -a Cauchy(a), 0 trivial.  out2 = {rho, c}
void yh_relpose_robust(const double* q1, const double* t1, const double* q2, const double* t2, const double* qo, const double* to, double w, const double* g3, double enc,
                       double* r, double* J1, double* J2, double* out2) {
    out2[0] = relpose_residual_ypr_robust<true>(mk(q1, t1), mk(q2, t2), mkm(qo, to, w), g3, enc, r, J1, J2, out2[1]);
}
void yh_relpose_robust_cost_only(const double* q1, const double* t1, const double* q2, const double* t2, const double* qo, const double* to, double w, const double* g3, double enc,
                                 double* r, double* out2) {
    out2[0] = relpose_residual_ypr_robust<false>(mk(q1, t1), mk(q2, t2), mkm(qo, to, w), g3, enc, r, nullptr, nullptr, out2[1]);
}
// the matrix-free product of one edge from its compact record: y1 / y2 by compact_apply at each side, b1 / b2 by compact_apply_both; rec22 returns the record
void yh_compact(const double* q1, const double* t1, const double* q2, const double* t2, const double* qo, const double* to, double w, const double* g3,
                const double* p1, const double* p2, double* y1, double* y2, double* b1, double* b2, double* rec22) {
    double rec[COMPACT_DOUBLES];
    edge_compact(mk(q1, t1), mk(q2, t2), mkm(qo, to, w), w, false, rec);
    if (g3[0] != 0.0) compact_mark_ypr(rec, g3);
    compact_apply<true>(rec, 0, p1, p2, 0.0, y1);
    compact_apply<true>(rec, 1, p2, p1, 0.0, y2);
    compact_apply_both<true>(rec, p1, p2, 0.0, b1, b2);
    for (int k = 0; k < COMPACT_DOUBLES; ++k) rec22[k] = rec[k];
}
// ... by the plain forms, which never look at the flag (what a handle without such an edge runs)
void yh_compact_plain(const double* q1, const double* t1, const double* q2, const double* t2, const double* qo, const double* to, double w, const double* p1, const double* p2, double* y1, double* y2) {
    double rec[COMPACT_DOUBLES];
    edge_compact(mk(q1, t1), mk(q2, t2), mkm(qo, to, w), w, false, rec);
    compact_apply(rec, 0, p1, p2, 0.0, y1);
    compact_apply(rec, 1, p2, p1, 0.0, y2);
}
}
