// Test-only host instantiation of the switchable block under a robust loss (csrc/pgo_device_math.hpp: switch_residual_robust, what K1's SWLOSS instantiations evaluate per
// lane) so that the corrected blocks can be checked without a GPU.  Not a product path.  With SWITCH_LOSS_HOST_MAIN it is a stand-alone program (own main): it reads a table of
// cases and expected values from the file named on its command line, evaluates every case and compares — the form that runs under -fsanitize=address,undefined.
#include "pgo_device_math.hpp"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
using namespace pgo;
static Pose mk(const double* q, const double* t) { return Pose{q[0], q[1], q[2], q[3], t[0], t[1], t[2]}; }
static Meas mkm(const double* T16, double w) {
    double R[9];
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) R[r * 3 + c] = T16[c * 4 + r];
    double q[4]; eigen_matrix_to_quat(R, q);
    return Meas{q[0], q[1], q[2], q[3], T16[12], T16[13], T16[14], w};
}
extern "C" {
// enc: +a Huber(a), -a Cauchy(a), 0 trivial.  The corrected block: r7, J1, J2 (6 x 6 each, the zero 7th row is not stored), Js7; out2 = {rho, c}
void sl_switch(const double* q1, const double* t1, const double* q2, const double* t2, double s, const double* T16, double w, double enc, double* r7, double* J1, double* J2, double* Js7, double* out2) {
    out2[0] = switch_residual_robust<true>(mk(q1, t1), mk(q2, t2), mkm(T16, w), s, enc, r7, J1, J2, Js7, out2[1]);
}
// ... as the cost-only instantiation evaluates it
void sl_switch_cost_only(const double* q1, const double* t1, const double* q2, const double* t2, double s, const double* T16, double w, double enc, double* r7, double* out2) {
    out2[0] = switch_residual_robust<false>(mk(q1, t1), mk(q2, t2), mkm(T16, w), s, enc, r7, nullptr, nullptr, nullptr, out2[1]);
}
// the plain block (switch_residual), for the bit-for-bit comparison at enc = 0
void sl_switch_plain(const double* q1, const double* t1, const double* q2, const double* t2, double s, const double* T16, double w, double* r7, double* J1, double* J2, double* Js7) {
    switch_residual<true>(mk(q1, t1), mk(q2, t2), mkm(T16, w), s, r7, J1, J2, Js7);
}
}

#ifdef SWITCH_LOSS_HOST_MAIN
// table file: a count n, then per case 33 inputs (q1[4] t1[3] q2[4] t2[3] s T16[16] w enc) and 88 expected values (rho c r7[7] J1[36] J2[36] Js7[7]), whitespace-separated
int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s <table>\n", argv[0]); return 2; }
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int n = 0;
    if (std::fscanf(f, "%d", &n) != 1 || n <= 0) { std::fclose(f); return 2; }
    double worst = 0.0;
    for (int k = 0; k < n; ++k) {
        std::vector<double> in(33), want(88), got(88);
        for (double& v : in) if (std::fscanf(f, "%lf", &v) != 1) { std::fclose(f); return 2; }
        for (double& v : want) if (std::fscanf(f, "%lf", &v) != 1) { std::fclose(f); return 2; }
        sl_switch(&in[0], &in[4], &in[7], &in[11], in[14], &in[15], in[31], in[32], &got[2], &got[9], &got[45], &got[81], &got[0]);
        std::vector<double> r7(7), o2(2);
        sl_switch_cost_only(&in[0], &in[4], &in[7], &in[11], in[14], &in[15], in[31], in[32], r7.data(), o2.data());
        if (std::memcmp(r7.data(), &got[2], 7 * sizeof(double)) != 0 || std::memcmp(o2.data(), &got[0], 2 * sizeof(double)) != 0) { std::printf("case %d: the cost-only form differs\n", k); std::fclose(f); return 1; }
        // groups: {rho}, {c}, r7, J1, J2, Js7 — each against its own largest expected magnitude (at least 1)
        const int lo[7] = {0, 1, 2, 9, 45, 81, 88};
        for (int g = 0; g < 6; ++g) {
            double scale = 1.0, err = 0.0;
            for (int i = lo[g]; i < lo[g + 1]; ++i) { scale = std::fmax(scale, std::fabs(want[i])); err = std::fmax(err, std::fabs(got[i] - want[i])); }
            worst = std::fmax(worst, err / scale);
        }
    }
    std::fclose(f);
    std::printf("cases %d worst relative error %.3e\n", n, worst);
    return worst <= 1e-12 ? 0 : 1;
}
#endif
