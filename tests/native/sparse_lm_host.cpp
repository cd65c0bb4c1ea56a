// Host side of pgo_sparse_lm_* (csrc/pgo_sparse_lm_math.hpp): the step plan, the damped Schur complement and right-hand side as the fill writes them into the permuted
// tiles, the whole exact LM step on ScHost (ScLmHost) and the solve loop (sc_lm_solve) around it with scripted callbacks.  Built as a shared object for
// tests/test_sparse_lm_host.py (tests/test_gpu_sparse_lm.py holds the kernels to it), or — with -DSLH_MAIN — as a stand-alone program that checks itself: the form to run
// under -fsanitize=address,undefined.
#include <cmath>
#include <cstring>
#include <string>

#include "pgo_sparse_lm_math.hpp"

namespace {
struct HostLm {
    int64_t N = 0; int used = 0;
    std::vector<uint8_t> in_system; std::vector<int32_t> hi, lo, order, pos;
    pgo::ScPlan P; pgo::ScLmPlan L;
    pgo::ScLmHost* H = nullptr;
    ~HostLm() { delete H; }
};
std::string g_error;

// The scripted problem of the controller test: a chain of N keyframes whose cost is a quadratic in the translations alone — a prior of weight 2 on keyframe 0,
// t_{i+1} - t_i = m_i per edge — and a unit block with zero gradient on every rotation, so that d_theta = 0 and the model is exact: every honest step has rho = 1.
// The script bends it: the `inflate`-th candidate evaluation reports a cost far above the present one (a rejected step), the `fail_eval`-th evaluate call fails, the
// `bad_lin`-th normal_blocks call returns a negative diagonal entry (a failed factorisation).
struct Quad {
    int64_t N; int inflate, fail_eval, bad_lin;
    int n_eval = 0, n_cand = 0, n_lin = 0;
    std::vector<double> t_lin;      // the point of the last evaluate that asked for a gradient
    double m(int64_t i, int k) const { return 0.5 + 0.25 * (double)((i * 3 + k) % 5); }
    double cost_of(const double* t, double* grad) const {
        double c = 0.0;
        if (grad) std::fill(grad, grad + N * 6, 0.0);
        for (int k = 0; k < 3; ++k) { const double r = 2.0 * (t[k] - 1.0); c += 0.5 * r * r; if (grad) grad[3 + k] += 2.0 * r; }
        for (int64_t i = 0; i + 1 < N; ++i)
            for (int k = 0; k < 3; ++k) { const double r = t[(i + 1) * 3 + k] - t[i * 3 + k] - m(i, k); c += 0.5 * r * r; if (grad) { grad[(i + 1) * 6 + 3 + k] += r; grad[i * 6 + 3 + k] -= r; } }
        return c;
    }
};
int quad_evaluate(void* user, const double*, const double* t, const double*, int64_t n_nodes, int64_t, double* cost, double*, double* gradient) {
    Quad& Q = *static_cast<Quad*>(user);
    if (n_nodes != Q.N) return PGO_ERR_INVALID_ARG;
    if (Q.n_eval++ == Q.fail_eval) return PGO_ERR_HIP;
    double c = Q.cost_of(t, gradient);
    if (gradient) Q.t_lin.assign(t, t + Q.N * 3);
    else if (Q.n_cand++ == Q.inflate) c = 10.0 * c + 100.0;
    if (cost) *cost = c;
    return PGO_OK;
}
int quad_normal_blocks(void* user, double* diag, double* grad, double* offdiag, double*, double*, double*) {
    Quad& Q = *static_cast<Quad*>(user);
    const bool bad = Q.n_lin++ == Q.bad_lin;
    std::fill(diag, diag + Q.N * 36, 0.0);
    for (int64_t i = 0; i < Q.N; ++i) {
        const double k = (i == 0 ? 4.0 : 0.0) + (i > 0 ? 1.0 : 0.0) + (i + 1 < Q.N ? 1.0 : 0.0);
        for (int a = 0; a < 3; ++a) { diag[i * 36 + a * 7] = 1.0; diag[i * 36 + (3 + a) * 7] = k; }
    }
    if (bad) diag[1 * 36 + 3 * 7] = -1e6;
    Q.cost_of(Q.t_lin.data(), grad);
    for (int64_t e = 0; e + 1 < Q.N; ++e) { std::fill(offdiag + e * 36, offdiag + e * 36 + 36, 0.0); for (int a = 3; a < 6; ++a) offdiag[e * 36 + a * 7] = -1.0; }
    return PGO_OK;
}
int quad_plus(void*, int64_t n, const double* q, const double* t, const double* d, double* qo, double* to) {
    for (int64_t i = 0; i < n; ++i) {
        const double* v = d + i * 6;
        const double th = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        if (th == 0.0) { std::copy(q + i * 4, q + i * 4 + 4, qo + i * 4); }
        else {      // [sin|d| d/|d| ; cos|d|] (x) q, quaternions x, y, z, w
            const double s = std::sin(th) / th, a[4] = {s * v[0], s * v[1], s * v[2], std::cos(th)}; const double* b = q + i * 4;
            qo[i * 4 + 0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
            qo[i * 4 + 1] = a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0];
            qo[i * 4 + 2] = a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3];
            qo[i * 4 + 3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
        }
        if (t && to) for (int k = 0; k < 3; ++k) to[i * 3 + k] = t[i * 3 + k] + v[3 + k];
    }
    return PGO_OK;
}
}  // namespace

extern "C" {
const char* slh_error() { return g_error.c_str(); }

// pgo_sparse_chol_create + pgo_sparse_lm_create on the host.  nullptr: refused, slh_error() says why.
void* slh_create(long long N, const unsigned char* in_system, const unsigned char* node_free, long long n_pairs, const int* hi, const int* lo, int ordering, long long n_rel, const int* rc1, const int* rc2,
                 long long n_sw, const int* sc1, const int* sc2) {
    g_error.clear();
    if (const char* what = pgo::sc_check_pairs(N, in_system, n_pairs, hi, lo)) { g_error = what; return nullptr; }
    HostLm* h = new HostLm;
    h->N = N; h->in_system.assign(in_system, in_system + N); h->hi.assign(hi, hi + n_pairs); h->lo.assign(lo, lo + n_pairs);
    std::vector<int64_t> adj_ptr; std::vector<int32_t> adj;
    pgo::sc_pair_adjacency(N, n_pairs, hi, lo, adj_ptr, adj);
    h->P = pgo::sc_plan_graph(N, adj_ptr.data(), adj.data(), in_system, ordering, h->order, &h->used);
    h->pos.assign((size_t)N, 0);
    for (long long q = 0; q < N; ++q) h->pos[(size_t)h->order[(size_t)q]] = (int32_t)q;
    h->L = pgo::ScLmPlan(N, in_system, node_free, n_pairs, h->hi.data(), h->lo.data(), n_rel, rc1, rc2, n_sw, sc1, sc2);
    if (h->L.error) { g_error = h->L.error; delete h; return nullptr; }
    h->H = new pgo::ScLmHost(h->L, h->P, h->pos.data(), h->hi.data(), h->lo.data());
    return h;
}
void slh_destroy(void* p) { delete static_cast<HostLm*>(p); }
// sizes6: entries of side, pair_ent, inc; nt; tiles of L; the ordering used
void slh_sizes(void* p, long long* sizes6, int* order) {
    const HostLm& h = *static_cast<HostLm*>(p);
    const long long v[6] = {(long long)h.L.side.size(), (long long)h.L.pair_ent.size(), (long long)h.L.inc.size(), h.P.nt, h.P.tiles(), h.used};
    std::copy(v, v + 6, sizes6);
    if (order) std::copy(h.order.begin(), h.order.end(), order);
}
void slh_plan(void* p, unsigned char* in_sys, int* side_ptr, int* side, int* pair_ptr, int* pair_ent, int* inc_ptr, int* inc) {
    const pgo::ScLmPlan& L = static_cast<HostLm*>(p)->L;
    std::copy(L.in_sys.begin(), L.in_sys.end(), in_sys);
    std::copy(L.side_ptr.begin(), L.side_ptr.end(), side_ptr); std::copy(L.side.begin(), L.side.end(), side);
    std::copy(L.pair_ptr.begin(), L.pair_ptr.end(), pair_ptr); std::copy(L.pair_ent.begin(), L.pair_ent.end(), pair_ent);
    std::copy(L.inc_ptr.begin(), L.inc_ptr.end(), inc_ptr); std::copy(L.inc.begin(), L.inc.end(), inc);
}
int slh_set_scale(void* p, const double* diag, const double* hss) { return static_cast<HostLm*>(p)->H->set_scale(diag, hss); }
// The system as the fill leaves it in the tiles, read back through the permutation: A [6 N][6 N] symmetric in the caller's keyframe order (identity on the rows of
// keyframes outside the system), b [6 N]; lam [6 N], a_inv [n_sw].  1: done; 0: a switch pivot is not > 0.
int slh_system(void* p, const double* diag, const double* grad, const double* off, const double* c, const double* hss, const double* gs, double radius, double mn, double mx, double* A, double* b,
               double* lam, double* a_inv) {
    HostLm& h = *static_cast<HostLm*>(p);
    pgo::ScLmHost& H = *h.H;
    const pgo::ScLmView V = H.view(diag, grad, off, c, hss, gs);
    const bool ok = H.assemble(V, radius, mn, mx);
    const long long n = h.N * 6;
    for (long long r = 0; r < n; ++r)
        for (long long q = 0; q <= r; ++q) {
            const int id = h.P.find((int)(r / pgo::DC_NB), (int)(q / pgo::DC_NB));
            const double v = id < 0 ? 0.0 : H.T[(size_t)id * pgo::SC_TILE + (size_t)(r % pgo::DC_NB) * pgo::DC_NB + q % pgo::DC_NB];
            const long long i = (long long)h.order[(size_t)(r / 6)] * 6 + r % 6, j = (long long)h.order[(size_t)(q / 6)] * 6 + q % 6;
            A[i * n + j] = A[j * n + i] = v;
        }
    for (long long r = 0; r < n; ++r) b[(long long)h.order[(size_t)(r / 6)] * 6 + r % 6] = H.w[(size_t)r];
    std::copy(H.lam.begin(), H.lam.end(), lam); std::copy(H.a_inv.begin(), H.a_inv.end(), a_inv);
    return ok ? 1 : 0;
}
int slh_step(void* p, const double* diag, const double* grad, const double* off, const double* c, const double* hss, const double* gs, double radius, double mn, double mx, double* dp, double* ds, double* out3) {
    return static_cast<HostLm*>(p)->H->step(diag, grad, off, c, hss, gs, radius, mn, mx, dp, ds, out3);
}

// sc_lm_solve on a chain of N keyframes with the scripted quadratic.  script3: inflate, fail_eval, bad_lin (-1: never).  opt12: max_num_iterations,
// max_num_consecutive_invalid_steps, initial / max / min trust-region radius, min_relative_decrease, function / gradient / parameter tolerance, min / max LM diagonal,
// jacobi_scaling.  t [3 N] in and out.  rec [9 per logged iteration]: valid, successful, reason, radius, relative decrease, cost, model cost change, step norm, cost change;
// meta4: logged iterations, termination type, num_iterations, calls of evaluate.  Returns sc_lm_solve's code.
int slh_scripted_solve(long long N, int ordering, const int* script3, const double* opt12, double* t, double* rec, double* meta4, char* message256) {
    std::vector<unsigned char> in((size_t)N, 1);
    std::vector<int> hi, lo;
    for (int i = 0; i + 1 < N; ++i) { hi.push_back(i + 1); lo.push_back(i); }
    void* hp = slh_create(N, in.data(), in.data(), (long long)hi.size(), hi.data(), lo.data(), ordering, (long long)hi.size(), lo.data(), hi.data(), 0, nullptr, nullptr);
    if (!hp) return PGO_ERR_INVALID_ARG;
    HostLm& h = *static_cast<HostLm*>(hp);
    pgo_options o;
    std::memset(&o, 0, sizeof(o));
    o.max_num_iterations = (int32_t)opt12[0]; o.max_num_consecutive_invalid_steps = (int32_t)opt12[1]; o.initial_trust_region_radius = opt12[2]; o.max_trust_region_radius = opt12[3];
    o.min_trust_region_radius = opt12[4]; o.min_relative_decrease = opt12[5]; o.function_tolerance = opt12[6]; o.gradient_tolerance = opt12[7]; o.parameter_tolerance = opt12[8];
    o.min_lm_diagonal = opt12[9]; o.max_lm_diagonal = opt12[10]; o.jacobi_scaling = (int32_t)opt12[11];
    Quad Q{N, script3[0], script3[1], script3[2]};
    std::vector<double> q((size_t)N * 4, 0.0);
    for (long long i = 0; i < N; ++i) q[(size_t)i * 4 + 3] = 1.0;
    const pgo::ScLmCallbacks cb{quad_evaluate, quad_normal_blocks, quad_plus};
    pgo_summary* sum = new pgo_summary;
    std::memset(sum, 0, sizeof(*sum));
    const int rc = pgo::sc_lm_solve(*h.H, h.L, cb, &Q, 0, nullptr, q.data(), t, nullptr, o, sum);
    for (int k = 0; k < sum->num_logged; ++k) {
        const pgo_iteration& it = sum->iterations[k];
        const double v[9] = {(double)it.step_is_valid, (double)it.step_is_successful, (double)it.reason, it.trust_region_radius, it.relative_decrease, it.cost, it.model_cost_change, it.step_norm, it.cost_change};
        std::copy(v, v + 9, rec + 9 * k);
        if (k > 0 && (it.preconditioner != PGO_PRECOND_DIRECT || it.cg_iterations != 0)) meta4[0] = -1.0;
    }
    if (meta4[0] != -1.0) meta4[0] = sum->num_logged;
    meta4[1] = sum->termination_type; meta4[2] = sum->num_iterations; meta4[3] = Q.n_eval;
    std::snprintf(message256, 256, "%s", sum->message);
    delete sum;
    slh_destroy(hp);
    return rc;
}
}

#ifdef SLH_MAIN
#include <cstdio>

static double lcg(unsigned long long& s) { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return (double)((s >> 11) & ((1ULL << 53) - 1)) / (double)(1ULL << 53) - 0.5; }

int main() {
    int bad = 0;
    // 9 keyframes: odometry 0-1-2-3-4-5-6-7, a second relative-pose edge on (1, 2) given as (2, 1), a switchable loop on (6, 1) beside nothing, one on (2, 1) beside the two
    // relative-pose edges, keyframe 4 constant, a switchable edge (4, 4 is refused, so:) between the constant keyframe 4 and the constant keyframe 5, keyframe 8 unreferenced
    const long long N = 9;
    const unsigned char free_[9] = {1, 1, 1, 1, 0, 0, 1, 1, 1}, insys[9] = {1, 1, 1, 1, 0, 0, 1, 1, 0};
    const int rc1[8] = {0, 1, 2, 3, 4, 5, 6, 2}, rc2[8] = {1, 2, 3, 4, 5, 6, 7, 1}, sc1[3] = {6, 2, 4}, sc2[3] = {1, 1, 5};
    const int hi[5] = {1, 1, 3, 7, 6}, lo[5] = {0, 2, 2, 6, 1};      // (the pair (1, 2) is named with the lower keyframe first)
    const long long n_rel = 8, n_sw = 3, E = 11;
    unsigned long long s = 11ULL;
    // normal blocks of random Jacobians: diag = sum J^T J (+ a prior on keyframe 0), offdiag = J1^T J2, c = [J1^T Js; J2^T Js], h = Js^T Js
    std::vector<double> diag((size_t)N * 36, 0.0), grad((size_t)N * 6, 0.0), off((size_t)E * 36, 0.0), c((size_t)n_sw * 12, 0.0), hss((size_t)n_sw, 0.0), gs((size_t)n_sw, 0.0);
    for (int a = 0; a < 6; ++a) diag[(size_t)a * 7] = 4.0;
    for (long long e = 0; e < E; ++e) {
        const bool sw = e >= n_rel;
        const int a = sw ? sc1[e - n_rel] : rc1[e], b = sw ? sc2[e - n_rel] : rc2[e];
        double J1[7][6], J2[7][6], Js[7], r[7];
        const int rows = sw ? 7 : 6;
        for (int i = 0; i < rows; ++i) { for (int k = 0; k < 6; ++k) { J1[i][k] = lcg(s) + (i == k ? 1.0 : 0.0); J2[i][k] = lcg(s) - (i == k ? 1.0 : 0.0); } Js[i] = lcg(s) + 1.0; r[i] = lcg(s); }
        for (int x = 0; x < 6; ++x) {
            for (int y = 0; y < 6; ++y) {
                double d1 = 0, d2 = 0, o = 0;
                for (int i = 0; i < rows; ++i) { d1 += J1[i][x] * J1[i][y]; d2 += J2[i][x] * J2[i][y]; o += J1[i][x] * J2[i][y]; }
                diag[(size_t)a * 36 + x * 6 + y] += d1; diag[(size_t)b * 36 + x * 6 + y] += d2; off[(size_t)e * 36 + x * 6 + y] = o;
            }
            double g1 = 0, g2 = 0, c1 = 0, c2 = 0;
            for (int i = 0; i < rows; ++i) { g1 += J1[i][x] * r[i]; g2 += J2[i][x] * r[i]; c1 += J1[i][x] * Js[i]; c2 += J2[i][x] * Js[i]; }
            grad[(size_t)a * 6 + x] += g1; grad[(size_t)b * 6 + x] += g2;
            if (sw) { c[(size_t)(e - n_rel) * 12 + x] = c1; c[(size_t)(e - n_rel) * 12 + 6 + x] = c2; }
        }
        if (sw) for (int i = 0; i < rows; ++i) { hss[(size_t)(e - n_rel)] += Js[i] * Js[i]; gs[(size_t)(e - n_rel)] += Js[i] * r[i]; }
    }
    for (int ordering : {0, 1}) {
        void* h = slh_create(N, insys, free_, 5, hi, lo, ordering, n_rel, rc1, rc2, n_sw, sc1, sc2);
        if (!h) { std::printf("ordering %d: refused: %s\n", ordering, slh_error()); ++bad; continue; }
        const int n = (int)N * 6;
        std::vector<double> A((size_t)n * n, 0.0), b((size_t)n), lam((size_t)n), ai((size_t)n_sw), dp((size_t)n, 7.0), ds((size_t)n_sw, 7.0);
        double out3[3];
        if (slh_step(h, diag.data(), grad.data(), off.data(), c.data(), hss.data(), gs.data(), 1e4, 1e-6, 1e32, dp.data(), ds.data(), out3) != PGO_ERR_STATE) { std::printf("a step without a scale was taken\n"); ++bad; }
        slh_set_scale(h, diag.data(), hss.data());
        if (!slh_system(h, diag.data(), grad.data(), off.data(), c.data(), hss.data(), gs.data(), 1e4, 1e-6, 1e32, A.data(), b.data(), lam.data(), ai.data())) { std::printf("ordering %d: a switch pivot failed\n", ordering); ++bad; }
        const int rc = slh_step(h, diag.data(), grad.data(), off.data(), c.data(), hss.data(), gs.data(), 1e4, 1e-6, 1e32, dp.data(), ds.data(), out3);
        if (rc != PGO_OK) { std::printf("ordering %d: the step failed (%d)\n", ordering, rc); ++bad; slh_destroy(h); continue; }
        double rmax = 0.0;
        for (int i = 0; i < n; ++i) {
            if (!insys[i / 6]) { if (dp[(size_t)i] != 0.0) { std::printf("ordering %d: an outside entry is not zero\n", ordering); ++bad; } continue; }
            double t = b[(size_t)i];
            for (int j = 0; j < n; ++j) t -= A[(size_t)i * n + j] * dp[(size_t)j];
            rmax = std::fmax(rmax, std::fabs(t));
        }
        std::printf("ordering %d: residual of the reduced system %.3e, model cost change %.6e, |d| %.3e\n", ordering, rmax, out3[0], out3[1]);
        if (!(rmax <= 1e-11) || !(out3[0] > 0.0)) ++bad;
        // an indefinite block: refused, and the next step gives the bits of the first
        std::vector<double> d2(diag), dq((size_t)n, 7.0), dt((size_t)n_sw, 7.0);
        d2[(size_t)2 * 36] = -50.0;
        double o3[3];
        if (slh_step(h, d2.data(), grad.data(), off.data(), c.data(), hss.data(), gs.data(), 1e4, 1e-6, 1e32, dq.data(), dt.data(), o3) != PGO_ERR_NUMERIC || dq[0] != 7.0) { std::printf("an indefinite block was accepted\n"); ++bad; }
        if (slh_step(h, diag.data(), grad.data(), off.data(), c.data(), hss.data(), gs.data(), 1e4, 1e-6, 1e32, dq.data(), dt.data(), o3) != PGO_OK || std::memcmp(dq.data(), dp.data(), dp.size() * sizeof(double)) != 0 ||
            std::memcmp(dt.data(), ds.data(), ds.size() * sizeof(double)) != 0 || o3[0] != out3[0]) { std::printf("the step after a failed one differs\n"); ++bad; }
        slh_destroy(h);
    }
    {   // refused plans: an edge on a pair the factor does not have; an edge from a keyframe to itself
        const int r1[9] = {0, 1, 2, 3, 4, 5, 6, 2, 0}, r2[9] = {1, 2, 3, 4, 5, 6, 7, 1, 3};
        if (slh_create(N, insys, free_, 5, hi, lo, 0, 9, r1, r2, n_sw, sc1, sc2)) { std::printf("an edge on no pair was accepted\n"); ++bad; }
        const int q1[9] = {0, 1, 2, 3, 4, 5, 6, 2, 3}, q2[9] = {1, 2, 3, 4, 5, 6, 7, 1, 3};
        if (slh_create(N, insys, free_, 5, hi, lo, 0, 9, q1, q2, n_sw, sc1, sc2)) { std::printf("a self edge was accepted\n"); ++bad; }
    }
    {   // the solve loop: an honest run, then a rejected step, a failed factorisation and a failing callback
        const double opt[12] = {50, 5, 1e4, 1e16, 1e-32, 1e-3, 1e-6, 1e-10, 1e-8, 1e-6, 1e32, 1};
        for (int which = 0; which < 4; ++which) {
            const int script[3] = {which == 1 ? 1 : -1, which == 3 ? 4 : -1, which == 2 ? 1 : -1};
            std::vector<double> t((size_t)12 * 3, 0.25), t0(t), rec((size_t)9 * PGO_MAX_ITERATION_LOG);
            double meta[4] = {0, 0, 0, 0};
            char msg[256];
            const int rc = slh_scripted_solve(12, which & 1, script, opt, t.data(), rec.data(), meta, msg);
            std::printf("script %d: rc %d, %d records, termination %d: %s\n", which, rc, (int)meta[0], (int)meta[1], msg);
            if (which == 3) { if (rc != PGO_ERR_HIP || t != t0) { std::printf("a failing callback did not end the solve untouched\n"); ++bad; } continue; }
            if (rc != PGO_OK || meta[1] != PGO_CONVERGENCE) ++bad;
            if (which == 1 && !(rec[9 * 2 + 0] == 1.0 && rec[9 * 2 + 1] == 0.0 && rec[9 * 2 + 2] == PGO_STEP_REJECTED_RHO)) { std::printf("the inflated candidate was not rejected\n"); ++bad; }
            if (which == 2 && !(rec[9 * 2 + 0] == 0.0 && rec[9 * 2 + 2] == PGO_STEP_INVALID_FACTORIZATION && rec[9 * 3 + 3] == 0.5 * rec[9 * 2 + 3])) { std::printf("the failed factorisation was not an invalid step\n"); ++bad; }
        }
    }
    std::printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}
#endif
