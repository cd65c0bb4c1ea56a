// Host side of pgo_sparse_yaw_graph_* (csrc/pgo_sparse_yaw_math.hpp): the graph model with its validation, the linearisation by the same per-item functions in the same
// orders as the kernels, run serially (SyHostLin), and the whole exact solve — sc_lm_solve over ScLmHost with this linearisation as its callbacks: a 4-DoF (yaw +
// translation) solve without a GPU.  Built as a shared object for tests/test_sparse_yaw_host.py (tests/test_gpu_sparse_yaw.py holds the kernels to it), or — with
// -DSYH_MAIN — as a stand-alone program that checks itself: the form to run under -fsanitize=address,undefined.
#include <cmath>
#include <cstring>
#include <string>

#include "pgo_sparse_lm_math.hpp"
#include "pgo_sparse_yaw_math.hpp"

namespace {
struct HostGraph {
    pgo::SyGraph G;
    pgo::SyHostLin L{G};
    std::string err;
    std::vector<double> far_yaw;      // of every evaluation of a solve: the largest |psi_j - psi_i - rel_yaw| over the edges, before the fold (0 without any)
};

double farthest_yaw(const pgo::SyGraph& G, const double* quat) {
    double far = 0.0;
    for (size_t e = 0; e < G.c1.size(); ++e) far = std::fmax(far, std::fabs(quat[4 * G.c2[e]] - quat[4 * G.c1[e]] - G.edge_num[e * pgo::SY_EDGE_DOUBLES + 3]));
    return far;
}

int cb_evaluate(void* user, const double* q, const double* t, const double*, int64_t n_nodes, int64_t, double* cost, double* residuals, double* gradient) {
    HostGraph& h = *static_cast<HostGraph*>(user);
    const int rc = h.L.evaluate(q, t, n_nodes, cost, residuals, gradient, h.err);
    if (rc == PGO_OK) h.far_yaw.push_back(farthest_yaw(h.G, q));
    return rc;
}
int cb_normal_blocks(void* user, double* diag, double* grad, double* offdiag, double*, double*, double*) {
    HostGraph& h = *static_cast<HostGraph*>(user);
    return h.L.normal_blocks(diag, grad, offdiag, h.err);
}
int cb_plus(void*, int64_t n, const double* q, const double* t, const double* d, double* qo, double* to) {
    for (int64_t i = 0; i < n; ++i) pgo::sy_plus_item(i, q, t, d, qo, to);
    return PGO_OK;
}
}  // namespace

extern "C" {
void* syh_create(long long n_nodes) {
    if (n_nodes < 1) return nullptr;
    HostGraph* h = new HostGraph;
    h->G.N = n_nodes;
    return h;
}
void syh_destroy(void* p) { delete static_cast<HostGraph*>(p); }
const char* syh_error(void* p) { return static_cast<HostGraph*>(p)->err.c_str(); }

int syh_add_edges(void* p, long long n, const int* c1, const int* c2, const double* t_meas, const double* rel_yaw, const double* pitch, const double* roll, const double* weight) {
    HostGraph& h = *static_cast<HostGraph*>(p);
    return h.G.add_edges(n, c1, c2, t_meas, rel_yaw, pitch, roll, weight, h.err);
}
int syh_set_nodes_constant(void* p, long long n, const int* node) {
    HostGraph& h = *static_cast<HostGraph*>(p);
    return h.G.set_constant(n, node, h.err);
}
int syh_finalize(void* p) {
    HostGraph& h = *static_cast<HostGraph*>(p);
    return h.G.finalize(h.err);
}
int syh_evaluate(void* p, const double* q, const double* t, long long n_nodes, double* cost, double* residuals, double* gradient) {
    HostGraph& h = *static_cast<HostGraph*>(p);
    return h.L.evaluate(q, t, n_nodes, cost, residuals, gradient, h.err);
}
int syh_normal_blocks(void* p, double* diag, double* grad, double* offdiag) {
    HostGraph& h = *static_cast<HostGraph*>(p);
    return h.L.normal_blocks(diag, grad, offdiag, h.err);
}
int syh_jacobian_blocks(void* p, long long first, long long count, double* J1, double* J2) {
    HostGraph& h = *static_cast<HostGraph*>(p);
    if (!h.L.linearised) { h.err = "no linearisation available (an evaluation with a gradient comes first)"; return PGO_ERR_STATE; }
    return pgo::sy_copy_jacobian_blocks(h.G.n_edges(), h.L.store.data(), first, count, J1, J2, h.err);
}
int syh_manifold_plus(void* p, long long n, const double* q, const double* t, const double* d, double* qo, double* to) { return cb_plus(p, n, q, t, d, qo, to); }
// counts3: n_nodes, n_edges, n_pairs; the lists as pgo_sparse_yaw_graph_edge_lists gives them (any may be NULL)
int syh_edge_lists(void* p, long long* counts3, unsigned char* node_free, unsigned char* in_system, int* c1, int* c2, int* pair_hi, int* pair_lo) {
    HostGraph& h = *static_cast<HostGraph*>(p);
    if (!h.G.finalized) { h.err = "before finalize"; return PGO_ERR_STATE; }
    if (counts3) { counts3[0] = h.G.N; counts3[1] = h.G.n_edges(); counts3[2] = (long long)h.G.pair_hi.size(); }
    if (node_free) std::copy(h.G.node_free.begin(), h.G.node_free.end(), node_free);
    if (in_system) std::copy(h.G.in_system.begin(), h.G.in_system.end(), in_system);
    if (c1) std::copy(h.G.c1.begin(), h.G.c1.end(), c1);
    if (c2) std::copy(h.G.c2.begin(), h.G.c2.end(), c2);
    if (pair_hi) std::copy(h.G.pair_hi.begin(), h.G.pair_hi.end(), pair_hi);
    if (pair_lo) std::copy(h.G.pair_lo.begin(), h.G.pair_lo.end(), pair_lo);
    return PGO_OK;
}

// One edge on its own: pose4 = psi (degrees), t; rec7 = t_meas, rel_yaw, pitch_i, roll_i, w.
void syh_residual(const double* pose_i, const double* pose_j, const double* rec7, double* r4, double* J1, double* J2) {
    pgo::sy_residual<true>(pose_i[0], pose_i[1], pose_i[2], pose_i[3], pose_j[0], pose_j[1], pose_j[2], pose_j[3], rec7, r4, J1, J2);
}
double syh_normalize(double a) { return pgo::sy_normalize(a); }

// pgo_sparse_chol_create + pgo_sparse_lm_create + pgo_sparse_lm_solve on the host, with this graph's linearisation as the callbacks.  options / summary: a pgo_options and a
// pgo_summary.  far_yaw [capacity]: the largest unfolded yaw argument over the edges at every evaluated point, *n_far of them.
int syh_solve(void* p, int ordering, double* quat, double* t, const void* options, void* summary, double* far_yaw, long long capacity, long long* n_far) {
    HostGraph& h = *static_cast<HostGraph*>(p);
    const pgo::SyGraph& G = h.G;
    if (!G.finalized) { h.err = "the graph is solved before finalize"; return PGO_ERR_STATE; }
    if (const int rc = G.check_state(quat, t, G.N, h.err)) return rc;
    const int64_t n_pairs = (int64_t)G.pair_hi.size();
    if (const char* what = pgo::sc_check_pairs(G.N, G.in_system.data(), n_pairs, G.pair_hi.data(), G.pair_lo.data())) { h.err = what; return PGO_ERR_INVALID_ARG; }
    std::vector<int64_t> adj_ptr; std::vector<int32_t> adj, order, pos((size_t)G.N, 0);
    int used = 0;
    pgo::sc_pair_adjacency(G.N, n_pairs, G.pair_hi.data(), G.pair_lo.data(), adj_ptr, adj);
    const pgo::ScPlan P = pgo::sc_plan_graph(G.N, adj_ptr.data(), adj.data(), G.in_system.data(), ordering, order, &used);
    for (int64_t q = 0; q < G.N; ++q) pos[(size_t)order[(size_t)q]] = (int32_t)q;
    const pgo::ScLmPlan L(G.N, G.in_system.data(), G.node_free.data(), n_pairs, G.pair_hi.data(), G.pair_lo.data(), G.n_edges(), G.c1.data(), G.c2.data(), 0, nullptr, nullptr);
    if (L.error) { h.err = L.error; return PGO_ERR_INVALID_ARG; }
    pgo::ScLmHost H(L, P, pos.data(), G.pair_hi.data(), G.pair_lo.data());
    const pgo::ScLmCallbacks cb{cb_evaluate, cb_normal_blocks, cb_plus};
    h.far_yaw.clear();
    const int rc = pgo::sc_lm_solve(H, L, cb, &h, 0, nullptr, quat, t, nullptr, *static_cast<const pgo_options*>(options), static_cast<pgo_summary*>(summary));
    if (n_far) *n_far = (long long)h.far_yaw.size();
    for (size_t k = 0; k < h.far_yaw.size() && (long long)k < capacity; ++k) far_yaw[k] = h.far_yaw[k];
    return rc;
}
}

#ifdef SYH_MAIN
#include <cstdio>

static double lcg(unsigned long long& s) { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return (double)((s >> 11) & ((1ULL << 53) - 1)) / (double)(1ULL << 53) - 0.5; }

// a chain of 12 keyframes on an arc that turns through 180 degrees, skips of 1 - 2, three loop closures, keyframe 0 constant; exact measurements, a start a few degrees and
// centimetres off: the solve must come back to the truth
int main() {
    int bad = 0;
    const int N = 12;
    unsigned long long s = 5ULL;
    std::vector<double> yaw((size_t)N), pitch((size_t)N), roll((size_t)N), q((size_t)N * 4, 0.0), t((size_t)N * 3);
    for (int i = 0; i < N; ++i) {
        yaw[(size_t)i] = pgo::sy_normalize(150.0 + 7.0 * i);      // 150 .. 227 -> crosses the fold
        pitch[(size_t)i] = 20.0 * lcg(s); roll[(size_t)i] = 20.0 * lcg(s);
        const double a = yaw[(size_t)i] / 180.0 * pgo::SY_PI;
        q[(size_t)i * 4] = yaw[(size_t)i];
        t[(size_t)i * 3] = 4.0 * std::sin(a); t[(size_t)i * 3 + 1] = -4.0 * std::cos(a); t[(size_t)i * 3 + 2] = 0.05 * i;
    }
    std::vector<int> c1, c2; std::vector<double> tm, ry, pi, ri;
    auto push = [&](int a, int b) {      // the exact measurement of the true state: r = 0 there
        double rec[7] = {0, 0, 0, 0, pitch[(size_t)a], roll[(size_t)a], 1.0}, r[4];
        pgo::sy_residual<false>(yaw[(size_t)a], t[(size_t)a * 3], t[(size_t)a * 3 + 1], t[(size_t)a * 3 + 2], yaw[(size_t)b], t[(size_t)b * 3], t[(size_t)b * 3 + 1], t[(size_t)b * 3 + 2], rec, r, nullptr, nullptr);
        c1.push_back(a); c2.push_back(b); tm.insert(tm.end(), r, r + 3); ry.push_back(pgo::sy_normalize(yaw[(size_t)b] - yaw[(size_t)a])); pi.push_back(pitch[(size_t)a]); ri.push_back(roll[(size_t)a]);
    };
    for (int i = 0; i < N; ++i) for (int k = 1; k <= 2; ++k) if (i + k < N) push(i, i + k);
    push(0, 9); push(10, 2); push(11, 4);
    void* h = syh_create(N);
    const long long E = (long long)c1.size();
    if (syh_add_edges(h, E, c1.data(), c2.data(), tm.data(), ry.data(), pi.data(), ri.data(), nullptr) != PGO_OK) { std::printf("edges refused: %s\n", syh_error(h)); ++bad; }
    {   // every refusal leaves the graph as it was
        const int a1[1] = {3}, far[1] = {N};
        const double nan1[3] = {0.0, NAN, 0.0}, inf1[1] = {INFINITY}, w0[1] = {0.0}, wn[1] = {-1.0}, one[3] = {1.0, 1.0, 1.0};
        if (syh_add_edges(h, 1, a1, a1, one, one, one, one, nullptr) != PGO_ERR_INVALID_ARG) { std::printf("a self edge was accepted\n"); ++bad; }
        if (syh_add_edges(h, 1, a1, far, one, one, one, one, nullptr) != PGO_ERR_INVALID_ARG) { std::printf("a keyframe out of range was accepted\n"); ++bad; }
        if (syh_add_edges(h, 1, c1.data(), c2.data(), nan1, one, one, one, nullptr) != PGO_ERR_INVALID_ARG) { std::printf("a non-finite measurement was accepted\n"); ++bad; }
        if (syh_add_edges(h, 1, c1.data(), c2.data(), one, inf1, one, one, nullptr) != PGO_ERR_INVALID_ARG) { std::printf("a non-finite yaw was accepted\n"); ++bad; }
        if (syh_add_edges(h, 1, c1.data(), c2.data(), one, one, one, one, w0) != PGO_ERR_INVALID_ARG) { std::printf("weight 0 was accepted\n"); ++bad; }
        if (syh_add_edges(h, 1, c1.data(), c2.data(), one, one, one, one, wn) != PGO_ERR_INVALID_ARG) { std::printf("a negative weight was accepted\n"); ++bad; }
        if (static_cast<HostGraph*>(h)->G.n_edges() != E) { std::printf("a refused call added edges\n"); ++bad; }
    }
    const int fixed[1] = {0};
    syh_set_nodes_constant(h, 1, fixed);
    double cost = 0.0;
    std::vector<double> q0(q), t0(t);
    if (syh_evaluate(h, q0.data(), t0.data(), N, &cost, nullptr, nullptr) != PGO_ERR_STATE) { std::printf("an evaluation before finalize ran\n"); ++bad; }
    if (syh_finalize(h) != PGO_OK) { std::printf("finalize failed: %s\n", syh_error(h)); ++bad; }
    if (syh_add_edges(h, 1, c1.data(), c2.data(), tm.data(), ry.data(), pi.data(), ri.data(), nullptr) != PGO_ERR_STATE) { std::printf("edges were added after finalize\n"); ++bad; }
    if (syh_evaluate(h, q0.data(), t0.data(), N, &cost, nullptr, nullptr) != PGO_OK || !(cost <= 1e-24)) { std::printf("the cost at the truth is %.3e\n", cost); ++bad; }
    q0[5] = 1e-3;
    if (syh_evaluate(h, q0.data(), t0.data(), N, &cost, nullptr, nullptr) != PGO_ERR_INVALID_ARG) { std::printf("a state with a non-zero pad slot was accepted\n"); ++bad; }
    q0[5] = 0.0;
    {   // a start a few degrees and centimetres off (keyframe 0 stays); the plus with t = NULL moves the yaw alone
        std::vector<double> d((size_t)N * 6, 0.0), qq(q0), tt(t0);
        for (int i = 1; i < N; ++i) { d[(size_t)i * 6] = 8.0 * lcg(s); for (int k = 3; k < 6; ++k) d[(size_t)i * 6 + k] = 0.1 * lcg(s); }
        syh_manifold_plus(h, N, qq.data(), tt.data(), d.data(), q0.data(), t0.data());
        std::vector<double> only((size_t)N * 4, -1.0);
        syh_manifold_plus(h, N, qq.data(), nullptr, d.data(), only.data(), nullptr);
        if (only != q0) { std::printf("the plus without t gives another yaw\n"); ++bad; }
        for (int i = 0; i < N; ++i) if (q0[(size_t)i * 4 + 1] != 0.0 || q0[(size_t)i * 4 + 2] != 0.0 || q0[(size_t)i * 4 + 3] != 0.0 || std::fabs(q0[(size_t)i * 4]) > 180.0) { std::printf("the plus left its layout\n"); ++bad; break; }
    }
    pgo_options o;
    std::memset(&o, 0, sizeof(o));
    o.max_num_iterations = 50; o.max_num_consecutive_invalid_steps = 5; o.initial_trust_region_radius = 1e4; o.max_trust_region_radius = 1e16; o.min_trust_region_radius = 1e-32;
    o.min_relative_decrease = 1e-3; o.function_tolerance = 1e-14; o.gradient_tolerance = 1e-10; o.parameter_tolerance = 1e-8; o.min_lm_diagonal = 1e-6; o.max_lm_diagonal = 1e32; o.jacobi_scaling = 1;
    pgo_summary* sum = new pgo_summary;
    std::memset(sum, 0, sizeof(*sum));
    std::vector<double> fy(256);
    long long n_fy = 0;
    const int rc = syh_solve(h, -1, q0.data(), t0.data(), &o, sum, fy.data(), 256, &n_fy);
    double far_t = 0.0, far_y = 0.0;
    for (int i = 0; i < N * 3; ++i) far_t = std::fmax(far_t, std::fabs(t0[(size_t)i] - t[(size_t)i]));
    for (int i = 0; i < N; ++i) far_y = std::fmax(far_y, std::fabs(pgo::sy_normalize(q0[(size_t)i * 4] - yaw[(size_t)i])));
    std::printf("solve: rc %d, termination %d, %d iterations, cost %.3e -> %.3e, %lld evaluations, max |t - truth| %.3e, max |yaw - truth| %.3e\n", rc, sum->termination_type, sum->num_iterations,
                sum->initial_cost, sum->final_cost, n_fy, far_t, far_y);
    if (rc != PGO_OK || sum->termination_type != PGO_CONVERGENCE || !(sum->final_cost <= 1e-12) || !(far_t <= 1e-5) || !(far_y <= 1e-4)) ++bad;
    delete sum;
    syh_destroy(h);
    std::printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}
#endif
