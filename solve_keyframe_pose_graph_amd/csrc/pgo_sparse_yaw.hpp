// pgo_sparse_yaw.hpp — the device side of pgo_sparse_yaw_graph (include/pgo_sparse.h), included at the end of pgo_sparse.hip: the companion library stays one translation
// unit.  The reference's 4-DoF pose graph (yaw in degrees + translation per keyframe, QinFourDOFWeightError on every edge) in the six-row slots of the exact LM step.  One
// linearisation (an evaluation that asks for a gradient):
//   sy_block_kernel<true>    one thread per edge (sy_block_item): the residual, J1 and J2 (4 x 4) into the block store, J1^T J2 into its 6 x 6 place of offdiag, 0.5 |r|^2
//                            into the workgroup's partial sum through the fixed binary tree of sg_block_kernel;
//   sg_cost_kernel           one workgroup: the partial sums in ascending order (pgo_sparse_graph.hpp's);
//   sy_node_kernel           one thread per keyframe (sy_node_item): diag and grad over the keyframe's incident list in list order, the unit pad entries.
// A cost-only evaluation is sy_block_kernel<false> and sg_cost_kernel.  sy_plus_kernel: one thread per keyframe.  The arithmetic is pgo_sparse_yaw_math.hpp's, shared with
// the host instantiation.  fp64 VALU, no atomics, one writer per address, nothing waits on another workgroup, every address from the tables of _finalize: two calls give the
// same bits.
#include "pgo_sparse_yaw_math.hpp"

namespace pgo {

namespace {

static_assert(SY_CHUNK == SC_THREADS, "one workgroup sums one chunk of cost terms");

template <bool WANT_J>
__global__ __launch_bounds__(SC_THREADS) void sy_block_kernel(SyView V, const double* __restrict__ quat, const double* __restrict__ t, SyOut O, double* __restrict__ part) {
    __shared__ double red[SC_THREADS];
    const int64_t e = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x;
    red[threadIdx.x] = e < V.E ? sy_block_item<WANT_J>(V, e, quat, t, O) : 0.0;
    __syncthreads();
    for (int s = SC_THREADS / 2; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

__global__ __launch_bounds__(SC_THREADS) void sy_node_kernel(SyView V, const double* __restrict__ store, const double* __restrict__ residuals, double* __restrict__ diag,
                                                             double* __restrict__ grad) {
    const int64_t node = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x;
    if (node < V.N) sy_node_item(V, node, store, residuals, diag, grad);
}

__global__ __launch_bounds__(SC_THREADS) void sy_plus_kernel(int64_t n, const double* __restrict__ quat, const double* __restrict__ t, const double* __restrict__ delta,
                                                             double* __restrict__ quat_out, double* __restrict__ t_out) {
    const int64_t i = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x;
    if (i < n) sy_plus_item(i, quat, t, delta, quat_out, t_out);
}

}  // namespace

}  // namespace pgo

struct pgo_sparse_yaw_graph {
    SyGraph G;
    int device = -1;
    hipStream_t st = nullptr;
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    DevBufs bufs;
    DevBuf tables{bufs}, num{bufs}, flags{bufs}, state{bufs}, lin{bufs}, tmp{bufs};
    SyView V{};                 // device pointers
    SyOut O{};
    double* d_diag = nullptr; double* d_grad = nullptr; double* d_part = nullptr; double* d_cost = nullptr;
    bool linearised = false;
    double ms[4] = {0, 0, 0, 0};      // of the last evaluation: upload, block kernel + cost reduction, node kernel, download
    int groups() const { return (int)sc_grid(std::max<int64_t>(V.E, 1)).x; }
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
int sy_cb_evaluate(void* user, const double* q, const double* t, const double*, int64_t n_nodes, int64_t, double* cost, double* residuals, double* gradient) {
    return pgo_sparse_yaw_graph_evaluate(static_cast<pgo_sparse_yaw_graph*>(user), q, t, n_nodes, cost, residuals, gradient);
}
int sy_cb_normal_blocks(void* user, double* diag, double* grad, double* offdiag, double*, double*, double*) {
    return pgo_sparse_yaw_graph_normal_blocks(static_cast<pgo_sparse_yaw_graph*>(user), diag, grad, offdiag);
}
int sy_cb_manifold_plus(void* user, int64_t n, const double* q, const double* t, const double* delta, double* qo, double* to) {
    return pgo_sparse_yaw_graph_manifold_plus(static_cast<pgo_sparse_yaw_graph*>(user), n, q, t, delta, qo, to);
}
}  // namespace

extern "C" {

int pgo_sparse_yaw_graph_create(int64_t n_nodes, int32_t device_id, pgo_sparse_yaw_graph** out) {
    g_err.clear();
    if (!out) { g_err = "pgo_sparse_yaw_graph_create: null pointer"; return PGO_ERR_INVALID_ARG; }
    *out = nullptr;
    if (n_nodes < 1 || n_nodes > (int64_t)300000000) { g_err = "pgo_sparse_yaw_graph_create: the number of keyframes is out of range"; return PGO_ERR_INVALID_ARG; }
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count < 1) { g_err = "no HIP device"; return PGO_ERR_NO_DEVICE; }
    if (device_id == -1 && hipGetDevice(&device_id) != hipSuccess) { g_err = "no current HIP device"; return PGO_ERR_NO_DEVICE; }
    if (device_id < 0 || device_id >= count) { g_err = "no such HIP device"; return PGO_ERR_NO_DEVICE; }
    pgo_sparse_yaw_graph* g = new pgo_sparse_yaw_graph;
    struct Guard { pgo_sparse_yaw_graph* g; ~Guard() { if (g) { g->release(); delete g; } } } guard{g};
    SCHIP(g_err, hipSetDevice(device_id));
    g->device = device_id;
    SCHIP(g_err, hipStreamCreate(&g->st));
    for (hipEvent_t& e : g->ev) SCHIP(g_err, hipEventCreate(&e));
    g->G.N = n_nodes;
    guard.g = nullptr;
    *out = g;
    return PGO_OK;
}

void pgo_sparse_yaw_graph_destroy(pgo_sparse_yaw_graph* g) {
    if (!g) return;
    g->release();
    delete g;
}

int pgo_sparse_yaw_graph_add_edges(pgo_sparse_yaw_graph* g, int64_t n, const int32_t* c1, const int32_t* c2, const double* t_meas, const double* rel_yaw, const double* pitch_i,
                                   const double* roll_i, const double* weight) {
    g_err.clear();
    if (!g) { g_err = "pgo_sparse_yaw_graph_add_edges: null pointer"; return PGO_ERR_INVALID_ARG; }
    std::string what;
    const int rc = g->G.add_edges(n, c1, c2, t_meas, rel_yaw, pitch_i, roll_i, weight, what);
    if (rc != PGO_OK) g_err = "pgo_sparse_yaw_graph_add_edges: " + what;
    return rc;
}

int pgo_sparse_yaw_graph_set_nodes_constant(pgo_sparse_yaw_graph* g, int64_t n, const int32_t* node) {
    g_err.clear();
    if (!g) { g_err = "pgo_sparse_yaw_graph_set_nodes_constant: null pointer"; return PGO_ERR_INVALID_ARG; }
    std::string what;
    const int rc = g->G.set_constant(n, node, what);
    if (rc != PGO_OK) g_err = "pgo_sparse_yaw_graph_set_nodes_constant: " + what;
    return rc;
}

int pgo_sparse_yaw_graph_finalize(pgo_sparse_yaw_graph* g) {
    g_err.clear();
    if (!g) { g_err = "pgo_sparse_yaw_graph_finalize: null pointer"; return PGO_ERR_INVALID_ARG; }
    std::string what;
    const int rc = g->G.finalize(what);
    if (rc != PGO_OK) { g_err = "pgo_sparse_yaw_graph_finalize: " + what; return rc; }
    SyGraph& G = g->G;
    struct Undo { SyGraph* G; ~Undo() { if (G) G->finalized = false; } } undo{&G};      // (an upload that fails leaves the graph as it was)
    SCHIP(g_err, hipSetDevice(g->device));
    const size_t N = (size_t)G.N, E = (size_t)G.n_edges();
    std::vector<int32_t> h;
    size_t at[4];
    const std::vector<int32_t>* parts[4] = {&G.c1, &G.c2, &G.inc_ptr, &G.inc};
    for (int k = 0; k < 4; ++k) { at[k] = h.size(); h.insert(h.end(), parts[k]->begin(), parts[k]->end()); }
    SCHIP(g_err, g->tables.ensure(h.size() * sizeof(int32_t)));
    SCHIP(g_err, hipMemcpy(g->tables.p, h.data(), h.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    SCHIP(g_err, g->num.ensure(std::max<size_t>(G.edge_num.size(), 1) * sizeof(double)));
    if (E) SCHIP(g_err, hipMemcpy(g->num.p, G.edge_num.data(), G.edge_num.size() * sizeof(double), hipMemcpyHostToDevice));
    SCHIP(g_err, g->flags.ensure(N));
    SCHIP(g_err, hipMemcpy(g->flags.p, G.node_free.data(), N, hipMemcpyHostToDevice));
    const int32_t* d = g->tables.as<int32_t>();
    g->V = SyView{G.N, (int64_t)E, d + at[0], d + at[1], g->num.as<double>(), g->flags.as<const uint8_t>(), d + at[2], d + at[3]};
    // one linearisation: residuals | store | offdiag | diag | grad | partial sums | cost
    const size_t groups = (size_t)g->groups();
    const size_t total = E * 4 + E * 32 + E * 36 + N * 36 + N * 6 + groups + 1;
    SCHIP(g_err, g->lin.ensure(total * sizeof(double)));
    double* p = g->lin.as<double>();
    g->O.residuals = p; p += E * 4;
    g->O.store = p; p += E * 32;
    g->O.offdiag = p; p += E * 36;
    g->d_diag = p; p += N * 36;
    g->d_grad = p; p += N * 6;
    g->d_part = p; p += groups;
    g->d_cost = p;
    undo.G = nullptr;
    return PGO_OK;
}

int pgo_sparse_yaw_graph_evaluate(pgo_sparse_yaw_graph* g, const double* quat, const double* t, int64_t n_nodes, double* cost, double* residuals, double* gradient) {
    g_err.clear();
    if (!g) { g_err = "pgo_sparse_yaw_graph_evaluate: null pointer"; return PGO_ERR_INVALID_ARG; }
    std::string what;
    const int rc = g->G.check_state(quat, t, n_nodes, what);
    if (rc != PGO_OK) { g_err = "pgo_sparse_yaw_graph_evaluate: " + what; return rc; }
    SCHIP(g_err, hipSetDevice(g->device));
    const size_t N = (size_t)n_nodes, E = (size_t)g->V.E;
    SCHIP(g_err, g->state.ensure(7 * N * sizeof(double)));
    double* dq = g->state.as<double>();
    double* dt = dq + 4 * N;
    hipStream_t st = g->st;
    SCHIP(g_err, hipEventRecord(g->ev[0], st));
    SCHIP(g_err, hipMemcpyAsync(dq, quat, 4 * N * sizeof(double), hipMemcpyHostToDevice, st));
    SCHIP(g_err, hipMemcpyAsync(dt, t, 3 * N * sizeof(double), hipMemcpyHostToDevice, st));
    SCHIP(g_err, hipEventRecord(g->ev[1], st));
    const dim3 grid((unsigned)g->groups());
    if (gradient) {
        g->linearised = false;
        hipLaunchKernelGGL((sy_block_kernel<true>), grid, dim3(SC_THREADS), 0, st, g->V, (const double*)dq, (const double*)dt, g->O, g->d_part);
    } else {      // the last linearisation's blocks stay what they are: a cost-only evaluation writes residuals (if asked for), partial sums and the cost alone
        SyOut O = g->O;
        if (!residuals) O.residuals = nullptr;
        hipLaunchKernelGGL((sy_block_kernel<false>), grid, dim3(SC_THREADS), 0, st, g->V, (const double*)dq, (const double*)dt, O, g->d_part);
    }
    hipLaunchKernelGGL(sg_cost_kernel, dim3(1), dim3(64), 0, st, (const double*)g->d_part, g->groups(), g->d_cost);
    SCHIP(g_err, hipEventRecord(g->ev[2], st));
    if (gradient) hipLaunchKernelGGL(sy_node_kernel, sc_grid(g->V.N), dim3(SC_THREADS), 0, st, g->V, (const double*)g->O.store, (const double*)g->O.residuals, g->d_diag, g->d_grad);
    SCHIP(g_err, hipEventRecord(g->ev[3], st));
    double h_cost = 0.0;
    SCHIP(g_err, hipMemcpyAsync(&h_cost, g->d_cost, sizeof(double), hipMemcpyDeviceToHost, st));
    if (residuals && E) SCHIP(g_err, hipMemcpyAsync(residuals, g->O.residuals, E * 4 * sizeof(double), hipMemcpyDeviceToHost, st));
    if (gradient) SCHIP(g_err, hipMemcpyAsync(gradient, g->d_grad, 6 * N * sizeof(double), hipMemcpyDeviceToHost, st));
    SCHIP(g_err, hipEventRecord(g->ev[4], st));
    SCHIP(g_err, hipStreamSynchronize(st));
    SCHIP(g_err, hipGetLastError());
    for (int k = 0; k < 4; ++k) { float ms = 0; SCHIP(g_err, hipEventElapsedTime(&ms, g->ev[k], g->ev[k + 1])); g->ms[k] = ms; }
    if (cost) *cost = h_cost;
    if (gradient) g->linearised = true;
    return PGO_OK;
}

int pgo_sparse_yaw_graph_normal_blocks(pgo_sparse_yaw_graph* g, double* diag, double* grad, double* offdiag) {
    g_err.clear();
    if (!g) { g_err = "pgo_sparse_yaw_graph_normal_blocks: null pointer"; return PGO_ERR_INVALID_ARG; }
    if (!g->linearised) { g_err = "pgo_sparse_yaw_graph_normal_blocks: no linearisation available (pgo_sparse_yaw_graph_evaluate with a gradient comes first)"; return PGO_ERR_STATE; }
    SCHIP(g_err, hipSetDevice(g->device));
    const size_t N = (size_t)g->V.N, E = (size_t)g->V.E;
    hipStream_t st = g->st;
    if (diag) SCHIP(g_err, hipMemcpyAsync(diag, g->d_diag, N * 36 * sizeof(double), hipMemcpyDeviceToHost, st));
    if (grad) SCHIP(g_err, hipMemcpyAsync(grad, g->d_grad, N * 6 * sizeof(double), hipMemcpyDeviceToHost, st));
    if (offdiag && E) SCHIP(g_err, hipMemcpyAsync(offdiag, g->O.offdiag, E * 36 * sizeof(double), hipMemcpyDeviceToHost, st));
    SCHIP(g_err, hipStreamSynchronize(st));
    return PGO_OK;
}

int pgo_sparse_yaw_graph_jacobian_blocks(pgo_sparse_yaw_graph* g, int64_t first, int64_t count, double* J1, double* J2) {
    g_err.clear();
    if (!g) { g_err = "pgo_sparse_yaw_graph_jacobian_blocks: null pointer"; return PGO_ERR_INVALID_ARG; }
    if (!g->linearised) { g_err = "pgo_sparse_yaw_graph_jacobian_blocks: no linearisation available (pgo_sparse_yaw_graph_evaluate with a gradient comes first)"; return PGO_ERR_STATE; }
    if (first < 0 || count < 0 || first + count > g->V.E) { g_err = "pgo_sparse_yaw_graph_jacobian_blocks: edges out of range"; return PGO_ERR_INVALID_ARG; }
    if (count == 0) return PGO_OK;
    SCHIP(g_err, hipSetDevice(g->device));
    std::vector<double> store((size_t)count * 32);
    SCHIP(g_err, hipMemcpyAsync(store.data(), g->O.store + first * 32, store.size() * sizeof(double), hipMemcpyDeviceToHost, g->st));
    SCHIP(g_err, hipStreamSynchronize(g->st));
    std::string what;
    return sy_copy_jacobian_blocks(count, store.data(), 0, count, J1, J2, what);
}

int pgo_sparse_yaw_graph_manifold_plus(pgo_sparse_yaw_graph* g, int64_t n, const double* quat, const double* t, const double* delta, double* quat_out, double* t_out) {
    g_err.clear();
    if (!g || n < 0 || (n > 0 && (!quat || !delta || !quat_out))) { g_err = "pgo_sparse_yaw_graph_manifold_plus: null pointer or negative count"; return PGO_ERR_INVALID_ARG; }
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
    hipLaunchKernelGGL(sy_plus_kernel, sc_grid(n), dim3(SC_THREADS), 0, st, n, (const double*)dq, with_t ? (const double*)dt : nullptr, (const double*)dd, dqo, with_t ? dto : nullptr);
    SCHIP(g_err, hipMemcpyAsync(quat_out, dqo, m * 4 * sizeof(double), hipMemcpyDeviceToHost, st));
    if (with_t) SCHIP(g_err, hipMemcpyAsync(t_out, dto, m * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
    SCHIP(g_err, hipStreamSynchronize(st));
    SCHIP(g_err, hipGetLastError());
    return PGO_OK;
}

int pgo_sparse_yaw_graph_lm_callbacks(pgo_sparse_yaw_graph* g, pgo_sparse_lm_callbacks* cb, void** user) {
    g_err.clear();
    if (!g || !cb || !user) { g_err = "pgo_sparse_yaw_graph_lm_callbacks: null pointer"; return PGO_ERR_INVALID_ARG; }
    cb->evaluate = sy_cb_evaluate; cb->normal_blocks = sy_cb_normal_blocks; cb->manifold_plus = sy_cb_manifold_plus;
    *user = g;
    return PGO_OK;
}

int pgo_sparse_yaw_graph_edge_lists(const pgo_sparse_yaw_graph* g, int64_t* counts3, uint8_t* node_free, uint8_t* in_system, int32_t* c1, int32_t* c2, int32_t* pair_hi, int32_t* pair_lo) {
    g_err.clear();
    if (!g) { g_err = "pgo_sparse_yaw_graph_edge_lists: null pointer"; return PGO_ERR_INVALID_ARG; }
    const SyGraph& G = g->G;
    if (!G.finalized) { g_err = "pgo_sparse_yaw_graph_edge_lists: before pgo_sparse_yaw_graph_finalize"; return PGO_ERR_STATE; }
    if (counts3) { counts3[0] = G.N; counts3[1] = G.n_edges(); counts3[2] = (int64_t)G.pair_hi.size(); }
    if (node_free) std::copy(G.node_free.begin(), G.node_free.end(), node_free);
    if (in_system) std::copy(G.in_system.begin(), G.in_system.end(), in_system);
    if (c1) std::copy(G.c1.begin(), G.c1.end(), c1);
    if (c2) std::copy(G.c2.begin(), G.c2.end(), c2);
    if (pair_hi) std::copy(G.pair_hi.begin(), G.pair_hi.end(), pair_hi);
    if (pair_lo) std::copy(G.pair_lo.begin(), G.pair_lo.end(), pair_lo);
    return PGO_OK;
}

int pgo_sparse_yaw_graph_last_times(const pgo_sparse_yaw_graph* g, double* ms4) {
    if (!g || !ms4) return PGO_ERR_INVALID_ARG;
    std::copy(g->ms, g->ms + 4, ms4);
    return PGO_OK;
}

}  // extern "C"
