// Test-only host instantiation of the robust-loss part of csrc/pgo_device_math.hpp (robust_loss, relpose_residual_robust: what K1's LOSS
// instantiations evaluate per lane) so that the loss values and the corrected blocks can be checked without a GPU.  Not a product path.
#include "pgo_device_math.hpp"
using namespace pgo;
extern "C" {
static Pose mk(const double* q, const double* t) { return Pose{q[0], q[1], q[2], q[3], t[0], t[1], t[2]}; }
static Meas mkm(const double* T16, double w) {
    double R[9];
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) R[r * 3 + c] = T16[c * 4 + r];
    double q[4]; eigen_matrix_to_quat(R, q);
    return Meas{q[0], q[1], q[2], q[3], T16[12], T16[13], T16[14], w};
}
// enc: +a Huber(a), -a Cauchy(a), 0 trivial.  out2 = {rho(s), sqrt(rho'(s))}
void rl_loss(double enc, double s, double* out2) { out2[0] = robust_loss(enc, s, out2[1]); }
// the corrected block; out2 = {rho, c}
void rl_relpose(const double* q1, const double* t1, const double* q2, const double* t2, const double* T16, double w, double enc, double* r, double* J1, double* J2, double* out2) {
    out2[0] = relpose_residual_robust<true>(mk(q1, t1), mk(q2, t2), mkm(T16, w), enc, r, J1, J2, out2[1]);
}
// ... as the cost-only instantiation evaluates it
void rl_relpose_cost_only(const double* q1, const double* t1, const double* q2, const double* t2, const double* T16, double w, double enc, double* r, double* out2) {
    out2[0] = relpose_residual_robust<false>(mk(q1, t1), mk(q2, t2), mkm(T16, w), enc, r, nullptr, nullptr, out2[1]);
}
}
