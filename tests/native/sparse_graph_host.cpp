// Host side of pgo_sparse_graph_* (csrc/pgo_sparse_graph_math.hpp): the graph model with its validation, the linearisation by the same per-item functions in the same orders as
// the kernels, run serially (SgHostLin), and the whole exact solve — sc_lm_solve over ScLmHost with this linearisation as its callbacks: a yaw/pitch/roll solve without a
// GPU.  Built as a shared object for tests/test_sparse_graph_host.py (tests/test_gpu_sparse_graph.py holds the kernels to it), or — with -DSGH_MAIN — as a stand-alone
// program that checks itself: the form to run under -fsanitize=address,undefined.
#include <cmath>
#include <cstring>
#include <string>

#include "pgo_sparse_graph_math.hpp"
#include "pgo_sparse_lm_math.hpp"

namespace {
struct HostGraph {
    pgo::SgGraph G;
    pgo::SgHostLin L{G};
    std::string err;
    std::vector<double> min_h;      // of every evaluation of a solve: the least h = cos(pitch error) over the yaw/pitch/roll-weighted edges (1 without any)
};

// h = sqrt(R00^2 + R10^2) of R(dq), dq = q2* (x) q1 (x) q_o: the cosine of the pitch error
double least_h(const pgo::SgGraph& G, const double* quat) {
    double least = 1.0;
    for (size_t e = 0; e < G.c1.size(); ++e) {
        const double* rec = &G.edge_num[e * pgo::SG_EDGE_DOUBLES];
        if (!(rec[8] > 0.0)) continue;
        const double* q1 = quat + 4 * G.c1[e];
        const double* q2 = quat + 4 * G.c2[e];
        const double q2c[4] = {-q2[0], -q2[1], -q2[2], q2[3]};
        double b[4], dq[4], R[9];
        pgo::quat_mul(q1, rec, b);
        pgo::quat_mul(q2c, b, dq);
        pgo::quat_to_rot(dq[0], dq[1], dq[2], dq[3], R);
        least = std::fmin(least, std::sqrt(R[0] * R[0] + R[3] * R[3]));
    }
    return least;
}

int cb_evaluate(void* user, const double* q, const double* t, const double* sw, int64_t n_nodes, int64_t n_switch, double* cost, double* residuals, double* gradient) {
    HostGraph& h = *static_cast<HostGraph*>(user);
    const int rc = h.L.evaluate(q, t, sw, n_nodes, n_switch, cost, residuals, gradient, h.err);
    if (rc == PGO_OK) h.min_h.push_back(least_h(h.G, q));
    return rc;
}
int cb_normal_blocks(void* user, double* diag, double* grad, double* offdiag, double* sw_c, double* sw_hss, double* sw_gs) {
    HostGraph& h = *static_cast<HostGraph*>(user);
    return h.L.normal_blocks(diag, grad, offdiag, sw_c, sw_hss, sw_gs, h.err);
}
int cb_plus(void*, int64_t n, const double* q, const double* t, const double* d, double* qo, double* to) {
    for (int64_t i = 0; i < n; ++i) pgo::sg_plus_item(i, q, t, d, qo, to);
    return PGO_OK;
}
}  // namespace

extern "C" {
void* sgh_create(long long n_nodes) {
    if (n_nodes < 1) return nullptr;
    HostGraph* h = new HostGraph;
    h->G.N = n_nodes;
    return h;
}
void sgh_destroy(void* p) { delete static_cast<HostGraph*>(p); }
const char* sgh_error(void* p) { return static_cast<HostGraph*>(p)->err.c_str(); }

int sgh_add_relpose_edges(void* p, long long n, const int* c1, const int* c2, const double* T, const double* w, const double* gains, int loss, double loss_a) {
    HostGraph& h = *static_cast<HostGraph*>(p);
    return h.G.add_relpose(n, c1, c2, T, w, gains, loss, loss_a, h.err);
}
int sgh_add_switchable_edges(void* p, long long n, const int* c1, const int* c2, const double* T, const int* idx, const double* gains, int loss, double loss_a) {
    HostGraph& h = *static_cast<HostGraph*>(p);
    return h.G.add_switchable(n, c1, c2, T, idx, gains, loss, loss_a, h.err);
}
int sgh_set_node_regularizers(void* p, long long n, const int* node, const double* target, const double* weight) {
    HostGraph& h = *static_cast<HostGraph*>(p);
    return h.G.set_priors(n, node, target, weight, h.err);
}
int sgh_set_nodes_constant(void* p, long long n, const int* node) {
    HostGraph& h = *static_cast<HostGraph*>(p);
    return h.G.set_constant(n, node, h.err);
}
int sgh_finalize(void* p) {
    HostGraph& h = *static_cast<HostGraph*>(p);
    return h.G.finalize(h.err);
}
int sgh_evaluate(void* p, const double* q, const double* t, const double* sw, long long n_nodes, long long n_switch, double* cost, double* residuals, double* gradient) {
    HostGraph& h = *static_cast<HostGraph*>(p);
    return h.L.evaluate(q, t, sw, n_nodes, n_switch, cost, residuals, gradient, h.err);
}
int sgh_normal_blocks(void* p, double* diag, double* grad, double* offdiag, double* sw_c, double* sw_hss, double* sw_gs) {
    HostGraph& h = *static_cast<HostGraph*>(p);
    return h.L.normal_blocks(diag, grad, offdiag, sw_c, sw_hss, sw_gs, h.err);
}
int sgh_jacobian_blocks(void* p, int kind, long long first, long long count, double* J1, double* J2, double* dr_ds) {
    HostGraph& h = *static_cast<HostGraph*>(p);
    if (!h.L.linearised) { h.err = "no linearisation available (an evaluation with a gradient comes first)"; return PGO_ERR_STATE; }
    return pgo::sg_copy_jacobian_blocks(h.G, h.L.store.data(), h.L.dr_ds.data(), kind, first, count, J1, J2, dr_ds, h.err);
}
int sgh_manifold_plus(void* p, long long n, const double* q, const double* t, const double* d, double* qo, double* to) { return cb_plus(p, n, q, t, d, qo, to); }
// counts6: n_nodes, n_rel, n_sw, n_pairs, the least n_switch, regularisers; the lists as pgo_sparse_graph_edge_lists gives them (any may be NULL)
int sgh_edge_lists(void* p, long long* counts6, unsigned char* node_free, unsigned char* in_system, int* pair_hi, int* pair_lo) {
    HostGraph& h = *static_cast<HostGraph*>(p);
    if (!h.G.finalized) { h.err = "before finalize"; return PGO_ERR_STATE; }
    const long long v[6] = {h.G.N, h.G.n_rel(), h.G.n_sw(), (long long)h.G.pair_hi.size(), h.G.min_switches(), h.G.n_prior()};
    if (counts6) std::copy(v, v + 6, counts6);
    if (node_free) std::copy(h.G.node_free.begin(), h.G.node_free.end(), node_free);
    if (in_system) std::copy(h.G.in_system.begin(), h.G.in_system.end(), in_system);
    if (pair_hi) std::copy(h.G.pair_hi.begin(), h.G.pair_hi.end(), pair_hi);
    if (pair_lo) std::copy(h.G.pair_lo.begin(), h.G.pair_lo.end(), pair_lo);
    return PGO_OK;
}

// One block of the switchable yaw/pitch/roll form on its own: pose7 = q (x, y, z, w), t; obs7 = q_obs, t_obs.  out2: rho, c.
void sgh_switch_ypr(const double* pose1, const double* pose2, const double* obs7, const double* gains, double s, double enc, double* r7, double* J1, double* J2, double* Js7, double* out2) {
    const pgo::Pose a{pose1[0], pose1[1], pose1[2], pose1[3], pose1[4], pose1[5], pose1[6]}, b{pose2[0], pose2[1], pose2[2], pose2[3], pose2[4], pose2[5], pose2[6]};
    const pgo::Meas m{obs7[0], obs7[1], obs7[2], obs7[3], obs7[4], obs7[5], obs7[6], 1.0};
    if (enc == 0.0) {
        pgo::switch_residual_ypr<true>(a, b, m, gains, s, r7, J1, J2, Js7);
        out2[0] = 0.0; for (int i = 0; i < 7; ++i) out2[0] += r7[i] * r7[i];
        out2[1] = 1.0;
    } else {
        out2[0] = pgo::switch_residual_ypr_robust<true>(a, b, m, gains, s, enc, r7, J1, J2, Js7, out2[1]);
    }
}

// pgo_sparse_chol_create + pgo_sparse_lm_create + pgo_sparse_lm_solve on the host, with this graph's linearisation as the callbacks.  options / summary: a pgo_options and a
// pgo_summary.  min_h [capacity]: the least cos(pitch error) over the yaw/pitch/roll edges at every evaluated point, *n_min_h of them.
int sgh_solve(void* p, int ordering, long long n_switch, double* quat, double* t, double* sw, const void* options, void* summary, double* min_h, long long capacity, long long* n_min_h) {
    HostGraph& h = *static_cast<HostGraph*>(p);
    const pgo::SgGraph& G = h.G;
    if (!G.finalized) { h.err = "the graph is solved before finalize"; return PGO_ERR_STATE; }
    const int64_t n_pairs = (int64_t)G.pair_hi.size();
    if (const char* what = pgo::sc_check_pairs(G.N, G.in_system.data(), n_pairs, G.pair_hi.data(), G.pair_lo.data())) { h.err = what; return PGO_ERR_INVALID_ARG; }
    std::vector<int64_t> adj_ptr; std::vector<int32_t> adj, order, pos((size_t)G.N, 0);
    int used = 0;
    pgo::sc_pair_adjacency(G.N, n_pairs, G.pair_hi.data(), G.pair_lo.data(), adj_ptr, adj);
    const pgo::ScPlan P = pgo::sc_plan_graph(G.N, adj_ptr.data(), adj.data(), G.in_system.data(), ordering, order, &used);
    for (int64_t q = 0; q < G.N; ++q) pos[(size_t)order[(size_t)q]] = (int32_t)q;
    const pgo::ScLmPlan L(G.N, G.in_system.data(), G.node_free.data(), n_pairs, G.pair_hi.data(), G.pair_lo.data(), G.n_rel(), G.rel_c1.data(), G.rel_c2.data(), G.n_sw(), G.sw_c1.data(), G.sw_c2.data());
    if (L.error) { h.err = L.error; return PGO_ERR_INVALID_ARG; }
    pgo::ScLmHost H(L, P, pos.data(), G.pair_hi.data(), G.pair_lo.data());
    const pgo::ScLmCallbacks cb{cb_evaluate, cb_normal_blocks, cb_plus};
    h.min_h.clear();
    const int rc = pgo::sc_lm_solve(H, L, cb, &h, n_switch, G.sw_idx.data(), quat, t, sw, *static_cast<const pgo_options*>(options), static_cast<pgo_summary*>(summary));
    if (n_min_h) *n_min_h = (long long)h.min_h.size();
    for (size_t k = 0; k < h.min_h.size() && (long long)k < capacity; ++k) min_h[k] = h.min_h[k];
    return rc;
}
}

#ifdef SGH_MAIN
#include <cstdio>

static double lcg(unsigned long long& s) { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return (double)((s >> 11) & ((1ULL << 53) - 1)) / (double)(1ULL << 53) - 0.5; }

// a chain of 12 keyframes on a gentle arc, f <= 2 odometry, three loop closures (one switchable), all yaw/pitch/roll-weighted, a regulariser on keyframe 0
int main() {
    int bad = 0;
    const int N = 12;
    unsigned long long s = 5ULL;
    std::vector<double> q((size_t)N * 4), t((size_t)N * 3);
    for (int i = 0; i < N; ++i) {
        const double a = 0.15 * i;
        q[(size_t)i * 4] = 0.0; q[(size_t)i * 4 + 1] = 0.0; q[(size_t)i * 4 + 2] = std::sin(a / 2); q[(size_t)i * 4 + 3] = std::cos(a / 2);
        t[(size_t)i * 3] = 4.0 * std::sin(a); t[(size_t)i * 3 + 1] = 4.0 * (1.0 - std::cos(a)); t[(size_t)i * 3 + 2] = 0.05 * i;
    }
    auto rel = [&](int a, int b, double* T) {      // c1_T_c2 of the true poses, column-major
        double Ra[9], Rb[9];
        pgo::quat_to_rot(q[(size_t)a * 4], q[(size_t)a * 4 + 1], q[(size_t)a * 4 + 2], q[(size_t)a * 4 + 3], Ra);
        pgo::quat_to_rot(q[(size_t)b * 4], q[(size_t)b * 4 + 1], q[(size_t)b * 4 + 2], q[(size_t)b * 4 + 3], Rb);
        std::fill(T, T + 16, 0.0); T[15] = 1.0;
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) { double v = 0; for (int k = 0; k < 3; ++k) v += Ra[k * 3 + r] * Rb[k * 3 + c]; T[c * 4 + r] = v; }
            double v = 0; for (int k = 0; k < 3; ++k) v += Ra[k * 3 + r] * (t[(size_t)b * 3 + k] - t[(size_t)a * 3 + k]);
            T[12 + r] = v;
        }
    };
    void* h = sgh_create(N);
    std::vector<int> c1, c2; std::vector<double> T, w, gains;
    auto push = [&](int a, int b) { c1.push_back(a); c2.push_back(b); T.resize(T.size() + 16); rel(a, b, &T[T.size() - 16]); w.push_back(1.0); for (double g : {4.0, 10.0, 10.0}) gains.push_back(g); };
    for (int i = 0; i < N; ++i) for (int k = 1; k <= 2; ++k) if (i + k < N) push(i, i + k);
    push(0, 9); push(10, 2);
    if (sgh_add_relpose_edges(h, (long long)c1.size(), c1.data(), c2.data(), T.data(), w.data(), gains.data(), PGO_LOSS_TRIVIAL, 0.0) != PGO_OK) { std::printf("edges refused: %s\n", sgh_error(h)); ++bad; }
    {   // every refusal leaves the graph as it was
        const int a1[1] = {3}, a2[1] = {3}, far[1] = {N};
        const double g_bad[3] = {4.0, 0.0, 10.0};
        std::vector<double> Tn(T.begin(), T.begin() + 16); Tn[5] = NAN;
        const long long before = (long long)static_cast<HostGraph*>(h)->G.n_rel();
        if (sgh_add_relpose_edges(h, 1, a1, a2, T.data(), w.data(), nullptr, 0, 0.0) != PGO_ERR_INVALID_ARG) { std::printf("a self edge was accepted\n"); ++bad; }
        if (sgh_add_relpose_edges(h, 1, a1, far, T.data(), w.data(), nullptr, 0, 0.0) != PGO_ERR_INVALID_ARG) { std::printf("a keyframe out of range was accepted\n"); ++bad; }
        if (sgh_add_relpose_edges(h, 1, c1.data(), c2.data(), T.data(), w.data(), g_bad, 0, 0.0) != PGO_ERR_INVALID_ARG) { std::printf("mixed gains were accepted\n"); ++bad; }
        if (sgh_add_relpose_edges(h, 1, c1.data(), c2.data(), T.data(), w.data(), nullptr, 7, 1.0) != PGO_ERR_INVALID_ARG) { std::printf("an unknown loss was accepted\n"); ++bad; }
        if (sgh_add_relpose_edges(h, 1, c1.data(), c2.data(), T.data(), w.data(), nullptr, PGO_LOSS_HUBER, 0.0) != PGO_ERR_INVALID_ARG) { std::printf("loss_a = 0 was accepted\n"); ++bad; }
        if (sgh_add_relpose_edges(h, 1, c1.data(), c2.data(), Tn.data(), w.data(), nullptr, 0, 0.0) != PGO_ERR_INVALID_ARG) { std::printf("a non-finite measurement was accepted\n"); ++bad; }
        if ((long long)static_cast<HostGraph*>(h)->G.n_rel() != before) { std::printf("a refused call added edges\n"); ++bad; }
    }
    const int s1[1] = {11}, s2[1] = {1}, si[1] = {0};
    double Ts[16]; rel(11, 1, Ts);
    const double gs3[3] = {4.0, 10.0, 10.0};
    if (sgh_add_switchable_edges(h, 1, s1, s2, Ts, si, gs3, PGO_LOSS_HUBER, 0.1) != PGO_OK) { std::printf("switchable edge refused: %s\n", sgh_error(h)); ++bad; }
    if (sgh_add_switchable_edges(h, 1, s1, s2, Ts, si, gs3, 0, 0.0) != PGO_ERR_INVALID_ARG) { std::printf("a switch index used twice was accepted\n"); ++bad; }
    const int reg[1] = {0};
    double Tr[16]; rel(0, 0, Tr);
    const double wr[1] = {2.0};
    sgh_set_node_regularizers(h, 1, reg, Tr, wr);
    double cost = 0.0;
    std::vector<double> q0(q), t0(t), sw(1, 0.99);
    if (sgh_evaluate(h, q0.data(), t0.data(), sw.data(), N, 1, &cost, nullptr, nullptr) != PGO_ERR_STATE) { std::printf("an evaluation before finalize ran\n"); ++bad; }
    if (sgh_finalize(h) != PGO_OK) { std::printf("finalize failed: %s\n", sgh_error(h)); ++bad; }
    if (sgh_add_relpose_edges(h, 1, c1.data(), c2.data(), T.data(), w.data(), nullptr, 0, 0.0) != PGO_ERR_STATE) { std::printf("edges were added after finalize\n"); ++bad; }
    {   // a start a few degrees and centimetres off
        std::vector<double> d((size_t)N * 6, 0.0), qq(q0), tt(t0);
        for (size_t k = 6; k < d.size(); ++k) d[k] = 0.04 * lcg(s);
        sgh_manifold_plus(h, N, qq.data(), tt.data(), d.data(), q0.data(), t0.data());
    }
    pgo_options o;
    std::memset(&o, 0, sizeof(o));
    o.max_num_iterations = 50; o.max_num_consecutive_invalid_steps = 5; o.initial_trust_region_radius = 1e4; o.max_trust_region_radius = 1e16; o.min_trust_region_radius = 1e-32;
    o.min_relative_decrease = 1e-3; o.function_tolerance = 1e-14; o.gradient_tolerance = 1e-10; o.parameter_tolerance = 1e-8; o.min_lm_diagonal = 1e-6; o.max_lm_diagonal = 1e32; o.jacobi_scaling = 1;
    pgo_summary* sum = new pgo_summary;
    std::memset(sum, 0, sizeof(*sum));
    std::vector<double> mh(256);
    long long n_mh = 0;
    const int rc = sgh_solve(h, -1, 1, q0.data(), t0.data(), sw.data(), &o, sum, mh.data(), 256, &n_mh);
    double least = 1.0, far = 0.0;
    for (long long k = 0; k < n_mh && k < 256; ++k) least = std::fmin(least, mh[(size_t)k]);
    for (int i = 0; i < N * 3; ++i) far = std::fmax(far, std::fabs(t0[(size_t)i] - t[(size_t)i]));
    std::printf("solve: rc %d, termination %d, %d iterations, cost %.3e -> %.3e, least cos(pitch error) %.4f, max |t - truth| %.3e\n", rc, sum->termination_type, sum->num_iterations, sum->initial_cost,
                sum->final_cost, least, far);
    if (rc != PGO_OK || sum->termination_type != PGO_CONVERGENCE || !(sum->final_cost <= 1e-12) || !(far <= 1e-5) || !(least >= 0.1736)) ++bad;
    delete sum;
    sgh_destroy(h);
    std::printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}
#endif
