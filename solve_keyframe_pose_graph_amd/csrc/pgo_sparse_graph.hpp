// pgo_sparse_graph.hpp — the device side of pgo_sparse_graph (include/pgo_sparse.h), included at the end of pgo_sparse.hip: the companion library stays one translation
// unit.  A pose graph with relative-pose, switchable and regulariser blocks — SixDOFError or yaw/pitch/roll-weighted, plain or robust — that linearises itself: no
// pgo_problem, no libpgo.so.  One linearisation (an evaluation that asks for a gradient):
//   sg_block_kernel<true, ..>   one thread per residual block (sg_block_item): the residual, J1, J2 and dr/ds into the block store, J1^T J2, the switch couplings, Js^T Js
//                               and Js^T r into their final places, 0.5 rho into the workgroup's partial sum through a fixed binary tree;
//   sg_cost_kernel              one workgroup: the partial sums in ascending order;
//   sg_node_kernel              one thread per keyframe (sg_node_item): diag and grad over the keyframe's incident list in list order.
// A cost-only evaluation is sg_block_kernel<false, ..> and sg_cost_kernel.  The arithmetic is pgo_sparse_graph_math.hpp's, shared with the host instantiation.  fp64 VALU,
// no atomics, one writer per address, nothing waits on another workgroup, every address from the tables of _finalize: two calls give the same bits.
#include "pgo_sparse_graph_math.hpp"

namespace pgo {

namespace {

static_assert(SG_CHUNK == SC_THREADS, "one workgroup sums one chunk of cost terms");

template <bool WANT_J, bool YPR, bool LOSS>
__global__ __launch_bounds__(SC_THREADS) void sg_block_kernel(SgView V, const double* __restrict__ quat, const double* __restrict__ t, const double* __restrict__ sw, SgOut O,
                                                              double* __restrict__ part) {
    __shared__ double red[SC_THREADS];
    const int64_t b = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x;
    red[threadIdx.x] = b < V.blocks() ? sg_block_item<WANT_J, YPR, LOSS>(V, b, quat, t, sw, O) : 0.0;
    __syncthreads();
    for (int s = SC_THREADS / 2; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

__global__ __launch_bounds__(64) void sg_cost_kernel(const double* __restrict__ part, int n, double* __restrict__ cost) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        double s = 0.0;
        for (int b = 0; b < n; ++b) s = s + part[b];
        *cost = s;
    }
}

__global__ __launch_bounds__(SC_THREADS) void sg_node_kernel(SgView V, const double* __restrict__ store, const double* __restrict__ residuals, double* __restrict__ diag,
                                                             double* __restrict__ grad) {
    const int64_t node = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x;
    if (node < V.N) sg_node_item(V, node, store, residuals, diag, grad);
}

__global__ __launch_bounds__(SC_THREADS) void sg_plus_kernel(int64_t n, const double* __restrict__ quat, const double* __restrict__ t, const double* __restrict__ delta,
                                                             double* __restrict__ quat_out, double* __restrict__ t_out) {
    const int64_t i = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x;
    if (i < n) sg_plus_item(i, quat, t, delta, quat_out, t_out);
}

template <bool WANT_J>
void sg_launch_blocks(bool ypr, bool loss, dim3 grid, hipStream_t st, const SgView& V, const double* q, const double* t, const double* sw, const SgOut& O, double* part) {
    if (ypr && loss) hipLaunchKernelGGL((sg_block_kernel<WANT_J, true, true>), grid, dim3(SC_THREADS), 0, st, V, q, t, sw, O, part);
    else if (ypr) hipLaunchKernelGGL((sg_block_kernel<WANT_J, true, false>), grid, dim3(SC_THREADS), 0, st, V, q, t, sw, O, part);
    else if (loss) hipLaunchKernelGGL((sg_block_kernel<WANT_J, false, true>), grid, dim3(SC_THREADS), 0, st, V, q, t, sw, O, part);
    else hipLaunchKernelGGL((sg_block_kernel<WANT_J, false, false>), grid, dim3(SC_THREADS), 0, st, V, q, t, sw, O, part);
}

}  // namespace

}  // namespace pgo

struct pgo_sparse_graph {
    SgGraph G;
    int device = -1;
    hipStream_t st = nullptr;
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    DevBufs bufs;
    DevBuf tables{bufs}, num{bufs}, flags{bufs}, state{bufs}, lin{bufs}, tmp{bufs};
    SgView V{};                 // device pointers
    SgOut O{};
    double* d_diag = nullptr; double* d_grad = nullptr; double* d_part = nullptr; double* d_cost = nullptr;
    std::vector<double> h_grad, h_gs;
    bool linearised = false;
    double ms[4] = {0, 0, 0, 0};      // of the last evaluation: upload, block kernel + cost reduction, node kernel, download
    int groups() const { return (int)sc_grid(std::max<int64_t>(V.blocks(), 1)).x; }
    void release() {
        if (device < 0) return;
        (void)hipSetDevice(device);
        if (st) (void)hipStreamSynchronize(st);
        release_all(bufs);
        for (hipEvent_t& e : ev) { if (e) (void)hipEventDestroy(e); e = nullptr; }
        if (st) (void)hipStreamDestroy(st);
        st = nullptr; device = -1;
    }
};

namespace {
int sg_cb_evaluate(void* user, const double* q, const double* t, const double* sw, int64_t n_nodes, int64_t n_switch, double* cost, double* residuals, double* gradient) {
    return pgo_sparse_graph_evaluate(static_cast<pgo_sparse_graph*>(user), q, t, sw, n_nodes, n_switch, cost, residuals, gradient);
}
int sg_cb_normal_blocks(void* user, double* diag, double* grad, double* offdiag, double* sw_c, double* sw_hss, double* sw_gs) {
    return pgo_sparse_graph_normal_blocks(static_cast<pgo_sparse_graph*>(user), diag, grad, offdiag, sw_c, sw_hss, sw_gs);
}
int sg_cb_manifold_plus(void* user, int64_t n, const double* q, const double* t, const double* delta, double* qo, double* to) {
    return pgo_sparse_graph_manifold_plus(static_cast<pgo_sparse_graph*>(user), n, q, t, delta, qo, to);
}
}  // namespace

extern "C" {

int pgo_sparse_graph_create(int64_t n_nodes, int32_t device_id, pgo_sparse_graph** out) {
    g_err.clear();
    if (!out) { g_err = "pgo_sparse_graph_create: null pointer"; return PGO_ERR_INVALID_ARG; }
    *out = nullptr;
    if (n_nodes < 1 || n_nodes > (int64_t)300000000) { g_err = "pgo_sparse_graph_create: the number of keyframes is out of range"; return PGO_ERR_INVALID_ARG; }
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count < 1) { g_err = "no HIP device"; return PGO_ERR_NO_DEVICE; }
    if (device_id == -1 && hipGetDevice(&device_id) != hipSuccess) { g_err = "no current HIP device"; return PGO_ERR_NO_DEVICE; }
    if (device_id < 0 || device_id >= count) { g_err = "no such HIP device"; return PGO_ERR_NO_DEVICE; }
    pgo_sparse_graph* g = new pgo_sparse_graph;
    struct Guard { pgo_sparse_graph* g; ~Guard() { if (g) { g->release(); delete g; } } } guard{g};
    SCHIP(g_err, hipSetDevice(device_id));
    g->device = device_id;
    SCHIP(g_err, hipStreamCreate(&g->st));
    for (hipEvent_t& e : g->ev) SCHIP(g_err, hipEventCreate(&e));
    g->G.N = n_nodes;
    guard.g = nullptr;
    *out = g;
    return PGO_OK;
}

void pgo_sparse_graph_destroy(pgo_sparse_graph* g) {
    if (!g) return;
    g->release();
    delete g;
}

int pgo_sparse_graph_add_relpose_edges(pgo_sparse_graph* g, int64_t n, const int32_t* c1, const int32_t* c2, const double* c1_T_c2, const double* weight, const double* ypr_gains, int32_t loss,
                                       double loss_a) {
    g_err.clear();
    if (!g) { g_err = "pgo_sparse_graph_add_relpose_edges: null pointer"; return PGO_ERR_INVALID_ARG; }
    std::string what;
    const int rc = g->G.add_relpose(n, c1, c2, c1_T_c2, weight, ypr_gains, loss, loss_a, what);
    if (rc != PGO_OK) g_err = "pgo_sparse_graph_add_relpose_edges: " + what;
    return rc;
}

int pgo_sparse_graph_add_switchable_edges(pgo_sparse_graph* g, int64_t n, const int32_t* c1, const int32_t* c2, const double* c1_T_c2, const int32_t* switch_idx, const double* ypr_gains,
                                          int32_t loss, double loss_a) {
    g_err.clear();
    if (!g) { g_err = "pgo_sparse_graph_add_switchable_edges: null pointer"; return PGO_ERR_INVALID_ARG; }
    std::string what;
    const int rc = g->G.add_switchable(n, c1, c2, c1_T_c2, switch_idx, ypr_gains, loss, loss_a, what);
    if (rc != PGO_OK) g_err = "pgo_sparse_graph_add_switchable_edges: " + what;
    return rc;
}

int pgo_sparse_graph_set_node_regularizers(pgo_sparse_graph* g, int64_t n, const int32_t* node, const double* target, const double* weight) {
    g_err.clear();
    if (!g) { g_err = "pgo_sparse_graph_set_node_regularizers: null pointer"; return PGO_ERR_INVALID_ARG; }
    std::string what;
    const int rc = g->G.set_priors(n, node, target, weight, what);
    if (rc != PGO_OK) g_err = "pgo_sparse_graph_set_node_regularizers: " + what;
    return rc;
}

int pgo_sparse_graph_set_nodes_constant(pgo_sparse_graph* g, int64_t n, const int32_t* node) {
    g_err.clear();
    if (!g) { g_err = "pgo_sparse_graph_set_nodes_constant: null pointer"; return PGO_ERR_INVALID_ARG; }
    std::string what;
    const int rc = g->G.set_constant(n, node, what);
    if (rc != PGO_OK) g_err = "pgo_sparse_graph_set_nodes_constant: " + what;
    return rc;
}

int pgo_sparse_graph_finalize(pgo_sparse_graph* g) {
    g_err.clear();
    if (!g) { g_err = "pgo_sparse_graph_finalize: null pointer"; return PGO_ERR_INVALID_ARG; }
    std::string what;
    const int rc = g->G.finalize(what);
    if (rc != PGO_OK) { g_err = "pgo_sparse_graph_finalize: " + what; return rc; }
    SgGraph& G = g->G;
    struct Undo { SgGraph* G; ~Undo() { if (G) G->finalized = false; } } undo{&G};      // (an upload that fails leaves the graph as it was)
    SCHIP(g_err, hipSetDevice(g->device));
    const size_t N = (size_t)G.N, Er = (size_t)G.n_rel(), Es = (size_t)G.n_sw(), Eg = (size_t)G.n_prior(), E = Er + Es, B = E + Eg;
    std::vector<int32_t> h;
    size_t at[6];
    const std::vector<int32_t>* parts[6] = {&G.c1, &G.c2, &G.sw_idx, &G.prior_node, &G.inc_ptr, &G.inc};
    for (int k = 0; k < 6; ++k) { at[k] = h.size(); h.insert(h.end(), parts[k]->begin(), parts[k]->end()); }
    SCHIP(g_err, g->tables.ensure(h.size() * sizeof(int32_t)));
    SCHIP(g_err, hipMemcpy(g->tables.p, h.data(), h.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    std::vector<double> nm(G.edge_num);
    nm.insert(nm.end(), G.prior_num.begin(), G.prior_num.end());
    SCHIP(g_err, g->num.ensure(nm.size() * sizeof(double)));
    if (!nm.empty()) SCHIP(g_err, hipMemcpy(g->num.p, nm.data(), nm.size() * sizeof(double), hipMemcpyHostToDevice));
    SCHIP(g_err, g->flags.ensure(N));
    SCHIP(g_err, hipMemcpy(g->flags.p, G.node_free.data(), N, hipMemcpyHostToDevice));
    const int32_t* d = g->tables.as<int32_t>();
    const double* dn = g->num.as<double>();
    g->V = SgView{G.N, (int64_t)Er, (int64_t)Es, (int64_t)Eg, d + at[0], d + at[1], d + at[2], d + at[3], dn, dn + E * SG_EDGE_DOUBLES, g->flags.as<const uint8_t>(), d + at[4], d + at[5]};
    // one linearisation: residuals | store | dr_ds | offdiag | sw_c | sw_hss | sw_gs | diag | grad | partial sums | cost
    const size_t R = (size_t)g->V.residuals(), groups = (size_t)g->groups();
    const size_t total = R + B * 72 + Es * 7 + E * 36 + Es * 12 + Es + Es + N * 36 + N * 6 + groups + 1;
    SCHIP(g_err, g->lin.ensure(total * sizeof(double)));
    double* p = g->lin.as<double>();
    g->O.residuals = p; p += R;
    g->O.store = p; p += B * 72;
    g->O.dr_ds = p; p += Es * 7;
    g->O.offdiag = p; p += E * 36;
    g->O.sw_c = p; p += Es * 12;
    g->O.sw_hss = p; p += Es;
    g->O.sw_gs = p; p += Es;
    g->d_diag = p; p += N * 36;
    g->d_grad = p; p += N * 6;
    g->d_part = p; p += groups;
    g->d_cost = p;
    g->h_grad.assign(N * 6, 0.0); g->h_gs.assign(Es, 0.0);
    undo.G = nullptr;
    return PGO_OK;
}

int pgo_sparse_graph_evaluate(pgo_sparse_graph* g, const double* quat, const double* t, const double* sw, int64_t n_nodes, int64_t n_switch, double* cost, double* residuals, double* gradient) {
    g_err.clear();
    if (!g) { g_err = "pgo_sparse_graph_evaluate: null pointer"; return PGO_ERR_INVALID_ARG; }
    std::string what;
    const int rc = g->G.check_state(quat, t, sw, n_nodes, n_switch, what);
    if (rc != PGO_OK) { g_err = "pgo_sparse_graph_evaluate: " + what; return rc; }
    SCHIP(g_err, hipSetDevice(g->device));
    const size_t N = (size_t)n_nodes, S = (size_t)n_switch, Es = (size_t)g->V.n_sw;
    SCHIP(g_err, g->state.ensure((7 * N + S) * sizeof(double)));
    double* dq = g->state.as<double>();
    double* dt = dq + 4 * N;
    double* ds = dt + 3 * N;
    hipStream_t st = g->st;
    SCHIP(g_err, hipEventRecord(g->ev[0], st));
    SCHIP(g_err, hipMemcpyAsync(dq, quat, 4 * N * sizeof(double), hipMemcpyHostToDevice, st));
    SCHIP(g_err, hipMemcpyAsync(dt, t, 3 * N * sizeof(double), hipMemcpyHostToDevice, st));
    if (S) SCHIP(g_err, hipMemcpyAsync(ds, sw, S * sizeof(double), hipMemcpyHostToDevice, st));
    SCHIP(g_err, hipEventRecord(g->ev[1], st));
    const dim3 grid((unsigned)g->groups());
    if (gradient) {
        g->linearised = false;
        sg_launch_blocks<true>(g->G.any_ypr, g->G.any_loss, grid, st, g->V, dq, dt, ds, g->O, g->d_part);
    } else {      // the last linearisation's blocks stay what they are: a cost-only evaluation writes residuals (if asked for), partial sums and the cost alone
        SgOut O = g->O;
        if (!residuals) O.residuals = nullptr;
        sg_launch_blocks<false>(g->G.any_ypr, g->G.any_loss, grid, st, g->V, dq, dt, ds, O, g->d_part);
    }
    hipLaunchKernelGGL(sg_cost_kernel, dim3(1), dim3(64), 0, st, (const double*)g->d_part, g->groups(), g->d_cost);
    SCHIP(g_err, hipEventRecord(g->ev[2], st));
    if (gradient) hipLaunchKernelGGL(sg_node_kernel, sc_grid(g->V.N), dim3(SC_THREADS), 0, st, g->V, (const double*)g->O.store, (const double*)g->O.residuals, g->d_diag, g->d_grad);
    SCHIP(g_err, hipEventRecord(g->ev[3], st));
    double h_cost = 0.0;
    SCHIP(g_err, hipMemcpyAsync(&h_cost, g->d_cost, sizeof(double), hipMemcpyDeviceToHost, st));
    if (residuals && g->V.residuals()) SCHIP(g_err, hipMemcpyAsync(residuals, g->O.residuals, (size_t)g->V.residuals() * sizeof(double), hipMemcpyDeviceToHost, st));
    if (gradient) {
        SCHIP(g_err, hipMemcpyAsync(gradient, g->d_grad, 6 * N * sizeof(double), hipMemcpyDeviceToHost, st));
        if (Es) SCHIP(g_err, hipMemcpyAsync(g->h_gs.data(), g->O.sw_gs, Es * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    SCHIP(g_err, hipEventRecord(g->ev[4], st));
    SCHIP(g_err, hipStreamSynchronize(st));
    SCHIP(g_err, hipGetLastError());
    for (int k = 0; k < 4; ++k) { float ms = 0; SCHIP(g_err, hipEventElapsedTime(&ms, g->ev[k], g->ev[k + 1])); g->ms[k] = ms; }
    if (cost) *cost = h_cost;
    if (gradient) {
        for (size_t i = 0; i < S; ++i) gradient[6 * N + i] = 0.0;
        for (size_t e = 0; e < Es; ++e) gradient[6 * N + (size_t)g->G.sw_idx[e]] = g->h_gs[e];
        g->linearised = true;
    }
    return PGO_OK;
}

int pgo_sparse_graph_normal_blocks(pgo_sparse_graph* g, double* diag, double* grad, double* offdiag, double* sw_c, double* sw_hss, double* sw_gs) {
    g_err.clear();
    if (!g) { g_err = "pgo_sparse_graph_normal_blocks: null pointer"; return PGO_ERR_INVALID_ARG; }
    if (!g->linearised) { g_err = "pgo_sparse_graph_normal_blocks: no linearisation available (pgo_sparse_graph_evaluate with a gradient comes first)"; return PGO_ERR_STATE; }
    SCHIP(g_err, hipSetDevice(g->device));
    const size_t N = (size_t)g->V.N, E = (size_t)(g->V.n_rel + g->V.n_sw), Es = (size_t)g->V.n_sw;
    hipStream_t st = g->st;
    if (diag) SCHIP(g_err, hipMemcpyAsync(diag, g->d_diag, N * 36 * sizeof(double), hipMemcpyDeviceToHost, st));
    if (grad) SCHIP(g_err, hipMemcpyAsync(grad, g->d_grad, N * 6 * sizeof(double), hipMemcpyDeviceToHost, st));
    if (offdiag && E) SCHIP(g_err, hipMemcpyAsync(offdiag, g->O.offdiag, E * 36 * sizeof(double), hipMemcpyDeviceToHost, st));
    if (sw_c && Es) SCHIP(g_err, hipMemcpyAsync(sw_c, g->O.sw_c, Es * 12 * sizeof(double), hipMemcpyDeviceToHost, st));
    if (sw_hss && Es) SCHIP(g_err, hipMemcpyAsync(sw_hss, g->O.sw_hss, Es * sizeof(double), hipMemcpyDeviceToHost, st));
    if (sw_gs && Es) SCHIP(g_err, hipMemcpyAsync(sw_gs, g->O.sw_gs, Es * sizeof(double), hipMemcpyDeviceToHost, st));
    SCHIP(g_err, hipStreamSynchronize(st));
    return PGO_OK;
}

int pgo_sparse_graph_jacobian_blocks(pgo_sparse_graph* g, int32_t kind, int64_t first, int64_t count, double* J1, double* J2, double* dr_ds) {
    g_err.clear();
    if (!g) { g_err = "pgo_sparse_graph_jacobian_blocks: null pointer"; return PGO_ERR_INVALID_ARG; }
    if (!g->linearised) { g_err = "pgo_sparse_graph_jacobian_blocks: no linearisation available (pgo_sparse_graph_evaluate with a gradient comes first)"; return PGO_ERR_STATE; }
    if (kind < 0 || kind > 2 || first < 0 || count < 0) { g_err = "pgo_sparse_graph_jacobian_blocks: unknown kind or negative range"; return PGO_ERR_INVALID_ARG; }
    const SgGraph& G = g->G;
    const int64_t n = kind == 0 ? G.n_rel() : kind == 1 ? G.n_sw() : G.n_prior();
    if (first + count > n) { g_err = "pgo_sparse_graph_jacobian_blocks: blocks out of range"; return PGO_ERR_INVALID_ARG; }
    if (count == 0) return PGO_OK;
    SCHIP(g_err, hipSetDevice(g->device));
    const int64_t b0 = (kind == 0 ? 0 : kind == 1 ? G.n_rel() : G.n_rel() + G.n_sw()) + first;
    std::vector<double> store((size_t)count * 72), dr(kind == 1 ? (size_t)count * 7 : 0);
    SCHIP(g_err, hipMemcpyAsync(store.data(), g->O.store + b0 * 72, store.size() * sizeof(double), hipMemcpyDeviceToHost, g->st));
    if (kind == 1) SCHIP(g_err, hipMemcpyAsync(dr.data(), g->O.dr_ds + first * 7, dr.size() * sizeof(double), hipMemcpyDeviceToHost, g->st));
    SCHIP(g_err, hipStreamSynchronize(g->st));
    for (int64_t k = 0; k < count; ++k) {
        const double* s = store.data() + k * 72;
        if (J1) std::copy(s, s + 36, J1 + k * 36);
        if (J2 && kind != 2) std::copy(s + 36, s + 72, J2 + k * 36);
    }
    if (dr_ds && kind == 1) std::copy(dr.begin(), dr.end(), dr_ds);
    return PGO_OK;
}

int pgo_sparse_graph_manifold_plus(pgo_sparse_graph* g, int64_t n, const double* quat, const double* t, const double* delta, double* quat_out, double* t_out) {
    g_err.clear();
    if (!g || n < 0 || (n > 0 && (!quat || !delta || !quat_out))) { g_err = "pgo_sparse_graph_manifold_plus: null pointer or negative count"; return PGO_ERR_INVALID_ARG; }
    if (n == 0) return PGO_OK;
    SCHIP(g_err, hipSetDevice(g->device));
    const bool with_t = t != nullptr && t_out != nullptr;
    const size_t m = (size_t)n;
    SCHIP(g_err, g->tmp.ensure(m * 20 * sizeof(double)));
    double* dq = g->tmp.as<double>();
    double* dd = dq + 4 * m; double* dqo = dd + 6 * m; double* dt = dqo + 4 * m; double* dto = dt + 3 * m;
    hipStream_t st = g->st;
    SCHIP(g_err, hipMemcpyAsync(dq, quat, m * 4 * sizeof(double), hipMemcpyHostToDevice, st));
    SCHIP(g_err, hipMemcpyAsync(dd, delta, m * 6 * sizeof(double), hipMemcpyHostToDevice, st));
    if (with_t) SCHIP(g_err, hipMemcpyAsync(dt, t, m * 3 * sizeof(double), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(sg_plus_kernel, sc_grid(n), dim3(SC_THREADS), 0, st, n, (const double*)dq, with_t ? (const double*)dt : nullptr, (const double*)dd, dqo, with_t ? dto : nullptr);
    SCHIP(g_err, hipMemcpyAsync(quat_out, dqo, m * 4 * sizeof(double), hipMemcpyDeviceToHost, st));
    if (with_t) SCHIP(g_err, hipMemcpyAsync(t_out, dto, m * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
    SCHIP(g_err, hipStreamSynchronize(st));
    SCHIP(g_err, hipGetLastError());
    return PGO_OK;
}

int pgo_sparse_graph_lm_callbacks(pgo_sparse_graph* g, pgo_sparse_lm_callbacks* cb, void** user) {
    g_err.clear();
    if (!g || !cb || !user) { g_err = "pgo_sparse_graph_lm_callbacks: null pointer"; return PGO_ERR_INVALID_ARG; }
    cb->evaluate = sg_cb_evaluate; cb->normal_blocks = sg_cb_normal_blocks; cb->manifold_plus = sg_cb_manifold_plus;
    *user = g;
    return PGO_OK;
}

int pgo_sparse_graph_edge_lists(const pgo_sparse_graph* g, int64_t* counts6, uint8_t* node_free, uint8_t* in_system, int32_t* rel_c1, int32_t* rel_c2, int32_t* swe_c1, int32_t* swe_c2,
                                int32_t* swe_index, int32_t* pair_hi, int32_t* pair_lo) {
    g_err.clear();
    if (!g) { g_err = "pgo_sparse_graph_edge_lists: null pointer"; return PGO_ERR_INVALID_ARG; }
    const SgGraph& G = g->G;
    if (!G.finalized) { g_err = "pgo_sparse_graph_edge_lists: before pgo_sparse_graph_finalize"; return PGO_ERR_STATE; }
    if (counts6) {
        const int64_t v[6] = {G.N, G.n_rel(), G.n_sw(), (int64_t)G.pair_hi.size(), G.min_switches(), G.n_prior()};
        std::copy(v, v + 6, counts6);
    }
    if (node_free) std::copy(G.node_free.begin(), G.node_free.end(), node_free);
    if (in_system) std::copy(G.in_system.begin(), G.in_system.end(), in_system);
    if (rel_c1) std::copy(G.rel_c1.begin(), G.rel_c1.end(), rel_c1);
    if (rel_c2) std::copy(G.rel_c2.begin(), G.rel_c2.end(), rel_c2);
    if (swe_c1) std::copy(G.sw_c1.begin(), G.sw_c1.end(), swe_c1);
    if (swe_c2) std::copy(G.sw_c2.begin(), G.sw_c2.end(), swe_c2);
    if (swe_index) std::copy(G.sw_idx.begin(), G.sw_idx.end(), swe_index);
    if (pair_hi) std::copy(G.pair_hi.begin(), G.pair_hi.end(), pair_hi);
    if (pair_lo) std::copy(G.pair_lo.begin(), G.pair_lo.end(), pair_lo);
    return PGO_OK;
}

int pgo_sparse_graph_last_times(const pgo_sparse_graph* g, double* ms4) {
    if (!g || !ms4) return PGO_ERR_INVALID_ARG;
    std::copy(g->ms, g->ms + 4, ms4);
    return PGO_OK;
}

}  // extern "C"
