// pgo_sparse_lm.hpp — the device side of pgo_sparse_lm_* (include/pgo_sparse.h), included at the end of pgo_sparse.hip: the companion library stays one translation unit.
// One LM system per pgo_sparse_lm_step: one upload of pgo_get_normal_blocks' arrays, then
//   sc_lm_scale_kernel     the damping of every pose column and the damped pivot of every switch (sc_lm_damp_column), one thread per column;
//   sc_lm_fill_kernel      the damped Schur complement straight into the zeroed tiles under the permutation, one thread per entry (sc_lm_fill_entry): each entry is a sum
//                          over the plan's CSR lists in list order, written once — no host reduction, no pair blocks in between;
//   sc_lm_rhs_kernel       the reduced right-hand side into the sweeps' W layout, one thread per row;
//   the factor and the two sweeps of pgo_sparse.hip, unchanged, through sc_factor_steps / sc_solve_steps;
//   sc_lm_backsub_kernel   dp back in the caller's keyframe order and ds;
//   sc_lm_model_kernel     d^T g, d^T H d and d^T d per keyframe and per switch (sc_lm_model_item), summed per workgroup by a fixed binary tree;
//   sc_lm_reduce_kernel    the workgroups' partial sums in ascending order, the model cost change and |d|;
// and one download.  The arithmetic is pgo_sparse_lm_math.hpp's, shared with the host instantiation.  No atomics, nothing waits on another workgroup, no MFMA here (the
// factor keeps it): 6 x 6 fp64 blocks gathered through the read-only path, one writer per address, every sum in a fixed order — two calls give the same bits.
#include "pgo_sparse_lm_math.hpp"

namespace pgo {

namespace {

__global__ __launch_bounds__(SC_THREADS) void sc_lm_scale_kernel(ScLmView V, double radius, double mn, double mx, int32_t* __restrict__ fail) {
    const int64_t j = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x;
    if (j >= V.N * 6 + V.n_sw) return;
    if (sc_lm_damp_column(V, j, radius, mn, mx)) *fail = 1;
}

// One thread per entry; a keyframe's six rows may straddle two tile rows and two tile columns (sc_block_entry gives the entry's own place), as in sc_fill_kernel
__global__ __launch_bounds__(SC_THREADS) void sc_lm_fill_kernel(double* __restrict__ T, ScDev P, ScLmView V) {
    const int64_t gid = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x;
    if (gid >= sc_lm_fill_threads(V)) return;
    int row, col;
    double v;
    if (!sc_lm_fill_entry(V, gid, &row, &col, &v)) return;
    const int id = sc_find(P, row / DC_NB, col / DC_NB);
    if (id < 0) return;                                                    // (the pattern was made from these very pairs)
    T[(size_t)id * SC_TILE + (size_t)(row % DC_NB) * DC_NB + col % DC_NB] = v;
}

// w [nc]: keyframe i's six entries at 6 pos[i] (pos is a permutation: every row below 6 N has one writer), zero outside the system and on the padding
__global__ __launch_bounds__(SC_THREADS) void sc_lm_rhs_kernel(ScLmView V, double* __restrict__ w) {
    const int64_t r = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x;
    if (r >= V.nc) return;
    if (r >= V.N * 6) { w[r] = 0.0; return; }
    const int64_t node = r / 6;
    const int a = (int)(r - node * 6);
    w[(size_t)V.pos[node] * 6 + a] = V.in_sys[node] ? sc_lm_rhs_entry(V, node, a) : 0.0;
}

__global__ __launch_bounds__(SC_THREADS) void sc_lm_backsub_kernel(ScLmView V, const double* __restrict__ x, double* __restrict__ dp, double* __restrict__ ds) {
    const int64_t r = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x;
    if (r < V.N * 6) {
        const int64_t node = r / 6;
        dp[r] = V.in_sys[node] ? x[(size_t)V.pos[node] * 6 + (r - node * 6)] : 0.0;
    } else if (r < V.N * 6 + V.n_sw) {
        const int64_t e = r - V.N * 6;
        ds[e] = sc_lm_backsub(V, e, x);
    }
}

static_assert(SC_LM_CHUNK == SC_THREADS, "one workgroup sums one chunk of the model's items");
// part [3 gridDim.x]: d^T g | d^T H d | d^T d of the workgroup's items
__global__ __launch_bounds__(SC_THREADS) void sc_lm_model_kernel(ScLmView V, const double* __restrict__ dp, const double* __restrict__ ds, double* __restrict__ part) {
    __shared__ double red[3][SC_THREADS];
    const int64_t it = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x;
    double g = 0.0, h = 0.0, n2 = 0.0;
    if (it < V.N + V.n_sw) sc_lm_model_item(V, it, dp, ds, &g, &h, &n2);
    red[0][threadIdx.x] = g; red[1][threadIdx.x] = h; red[2][threadIdx.x] = n2;
    __syncthreads();
    for (int s = SC_THREADS / 2; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s)
            for (int k = 0; k < 3; ++k) red[k][threadIdx.x] = red[k][threadIdx.x] + red[k][threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x < 3) part[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = red[threadIdx.x][0];
}
// one workgroup: thread k < 3 sums quantity k over the n partial sums in ascending order; out3[0] = model cost change, out3[1] = |d|
__global__ __launch_bounds__(64) void sc_lm_reduce_kernel(const double* __restrict__ part, int n, double* __restrict__ out3) {
    __shared__ double tot[3];
    if (threadIdx.x < 3) {
        double s = 0.0;
        for (int b = 0; b < n; ++b) s = s + part[(size_t)threadIdx.x * n + b];
        tot[threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) { out3[0] = sc_lm_model_cost_change(tot[0], tot[1]); out3[1] = sqrt(tot[2]); out3[2] = 0.0; }
}

}  // namespace

}  // namespace pgo

struct pgo_sparse_lm {
    pgo_sparse_chol* chol = nullptr;
    ScLmPlan plan;
    ScLmView V{};                                          // device pointers
    DevBufs bufs;
    DevBuf tables{bufs}, d_insys{bufs}, num{bufs}, scale{bufs}, out{bufs}, part{bufs};
    std::vector<double> h_scale, stage, h_out;
    bool scale_set = false;
    hipEvent_t ev[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    double ms[6] = {0, 0, 0, 0, 0, 0};                     // upload, scale + fill + rhs, factor, sweeps, back-substitution + model, download
    int blocks() const { return (int)sc_grid(plan.N + plan.n_sw).x; }
    void release() {
        if (chol && chol->c.device >= 0) (void)hipSetDevice(chol->c.device);
        if (chol && chol->c.st) (void)hipStreamSynchronize(chol->c.st);
        release_all(bufs);
        for (hipEvent_t& e : ev) { if (e) (void)hipEventDestroy(e); e = nullptr; }
    }
};

namespace {
struct ScLmDeviceStepper {
    pgo_sparse_lm* lm;
    int set_scale(const double* diag, const double* sw_hss) { return pgo_sparse_lm_set_scale(lm, diag, sw_hss); }
    int step(const double* diag, const double* grad, const double* offdiag, const double* sw_c, const double* sw_hss, const double* sw_gs, double radius, double mn, double mx, double* dp, double* ds, double* out3) {
        return pgo_sparse_lm_step(lm, diag, grad, offdiag, sw_c, sw_hss, sw_gs, radius, mn, mx, dp, ds, out3);
    }
};
}  // namespace

extern "C" {

int pgo_sparse_lm_create(pgo_sparse_chol* chol, int64_t n_nodes, const uint8_t* node_free, int64_t n_rel, const int32_t* rel_c1, const int32_t* rel_c2, int64_t n_sw, const int32_t* swe_c1,
                         const int32_t* swe_c2, pgo_sparse_lm** out) {
    g_err.clear();
    if (!out) { g_err = "pgo_sparse_lm_create: null pointer"; return PGO_ERR_INVALID_ARG; }
    *out = nullptr;
    if (!chol || !node_free || n_nodes != chol->N || n_rel < 0 || n_sw < 0 || (n_rel > 0 && (!rel_c1 || !rel_c2)) || (n_sw > 0 && (!swe_c1 || !swe_c2))) {
        g_err = "pgo_sparse_lm_create: null pointer, negative count, or n_nodes is not the factor's"; return PGO_ERR_INVALID_ARG;
    }
    pgo_sparse_lm* lm = new pgo_sparse_lm;
    struct Guard { pgo_sparse_lm* lm; std::string* err; ~Guard() { if (lm) { g_err = *err; lm->release(); delete lm; } } } guard{lm, &chol->c.err};
    lm->chol = chol;
    ScCore& c = chol->c;
    c.err.clear();
    lm->plan = ScLmPlan(n_nodes, chol->in_system.data(), node_free, chol->n_pairs, chol->h_hi.data(), chol->h_lo.data(), n_rel, rel_c1, rel_c2, n_sw, swe_c1, swe_c2);
    if (lm->plan.error) { c.err = std::string("pgo_sparse_lm_create: ") + lm->plan.error; return PGO_ERR_INVALID_ARG; }
    int rc;
    if ((rc = c.use()) != PGO_OK) return rc;
    const ScLmPlan& L = lm->plan;
    const size_t N = (size_t)L.N, E = (size_t)(L.n_rel + L.n_sw), Es = (size_t)L.n_sw;
    std::vector<int32_t> h;
    size_t at[8];
    const std::vector<int32_t>* parts[8] = {&L.side_ptr, &L.side, &L.pair_ptr, &L.pair_ent, &L.inc_ptr, &L.inc, &L.c1, &L.c2};
    for (int k = 0; k < 8; ++k) { at[k] = h.size(); h.insert(h.end(), parts[k]->begin(), parts[k]->end()); }
    SCHIP(c.err, lm->tables.ensure(h.size() * sizeof(int32_t)));
    SCHIP(c.err, hipMemcpy(lm->tables.p, h.data(), h.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    SCHIP(c.err, lm->d_insys.ensure(N));
    SCHIP(c.err, hipMemcpy(lm->d_insys.p, L.in_sys.data(), N, hipMemcpyHostToDevice));
    const size_t n_num = N * 42 + E * 36 + Es * 14, n_scale = 2 * (N * 6 + Es), n_out = N * 6 + Es + 3;
    SCHIP(c.err, lm->num.ensure(n_num * sizeof(double))); SCHIP(c.err, lm->scale.ensure(n_scale * sizeof(double)));
    SCHIP(c.err, lm->out.ensure(n_out * sizeof(double))); SCHIP(c.err, lm->part.ensure((size_t)3 * lm->blocks() * sizeof(double)));
    SCHIP(c.err, c.vec.ensure((size_t)3 * c.nc() * sizeof(double)));
    for (hipEvent_t& e : lm->ev) SCHIP(c.err, hipEventCreate(&e));
    lm->stage.assign(n_num, 0.0); lm->h_out.assign(n_out, 0.0); lm->h_scale.assign(N * 6 + Es, 1.0);
    const int32_t* d = lm->tables.as<int32_t>();
    const double* nm = lm->num.as<double>();
    double* sc = lm->scale.as<double>();
    lm->V = ScLmView{L.N, L.n_rel, L.n_sw, L.n_pairs, c.nc(), lm->d_insys.as<const uint8_t>(), chol->d_pos.as<const int32_t>(), d + at[0], d + at[1], d + at[2], d + at[3],
                     chol->d_hi.as<const int32_t>(), chol->d_lo.as<const int32_t>(), d + at[4], d + at[5], d + at[6], d + at[7],
                     nm, nm + N * 36, nm + N * 42, nm + N * 42 + E * 36, nm + N * 42 + E * 36 + Es * 12, nm + N * 42 + E * 36 + Es * 13,
                     sc, sc + N * 6, sc + N * 6 + Es, sc + 2 * N * 6 + Es};
    guard.lm = nullptr;
    *out = lm;
    return PGO_OK;
}

void pgo_sparse_lm_destroy(pgo_sparse_lm* lm) {
    if (!lm) return;
    lm->release();
    delete lm;
}

int pgo_sparse_lm_set_scale(pgo_sparse_lm* lm, const double* diag, const double* sw_hss) {
    if (!lm) return PGO_ERR_INVALID_ARG;
    ScCore& c = lm->chol->c;
    c.err.clear();
    const ScLmPlan& L = lm->plan;
    if (diag && L.n_sw > 0 && !sw_hss) { c.err = "pgo_sparse_lm_set_scale: null pointer"; return PGO_ERR_INVALID_ARG; }
    int rc;
    if ((rc = c.use()) != PGO_OK) return rc;
    for (int64_t j = 0; j < L.N * 6; ++j) lm->h_scale[(size_t)j] = diag ? sc_lm_scale(diag[(j / 6) * 36 + (j % 6) * 7]) : 1.0;
    for (int64_t e = 0; e < L.n_sw; ++e) lm->h_scale[(size_t)(L.N * 6 + e)] = diag ? sc_lm_scale(sw_hss[e]) : 1.0;
    SCHIP(c.err, hipMemcpyAsync(lm->scale.p, lm->h_scale.data(), lm->h_scale.size() * sizeof(double), hipMemcpyHostToDevice, c.st));
    SCHIP(c.err, hipStreamSynchronize(c.st));
    lm->scale_set = true;
    return PGO_OK;
}

int pgo_sparse_lm_step(pgo_sparse_lm* lm, const double* diag, const double* grad, const double* offdiag, const double* sw_c, const double* sw_hss, const double* sw_gs, double radius,
                       double min_lm_diagonal, double max_lm_diagonal, double* delta_pose, double* delta_sw, double* out3) {
    if (!lm) return PGO_ERR_INVALID_ARG;
    pgo_sparse_chol* h = lm->chol;
    ScCore& c = h->c;
    c.err.clear();
    const ScLmPlan& L = lm->plan;
    const size_t N = (size_t)L.N, E = (size_t)(L.n_rel + L.n_sw), Es = (size_t)L.n_sw;
    if (!diag || !grad || !delta_pose || !out3 || (E > 0 && !offdiag) || (Es > 0 && (!sw_c || !sw_hss || !sw_gs || !delta_sw))) { c.err = "pgo_sparse_lm_step: null pointer"; return PGO_ERR_INVALID_ARG; }
    if (!(radius > 0.0)) { c.err = "pgo_sparse_lm_step: the radius is not > 0"; return PGO_ERR_INVALID_ARG; }
    if (!lm->scale_set) { c.err = "pgo_sparse_lm_step: no scale (pgo_sparse_lm_set_scale comes first)"; return PGO_ERR_STATE; }
    int rc;
    if ((rc = c.use()) != PGO_OK) return rc;
    h->factored = false; h->selected = false;              // (the tiles are about to hold the factor of a damped system)
    double* st = lm->stage.data();
    std::copy(diag, diag + N * 36, st); std::copy(grad, grad + N * 6, st + N * 36);
    if (E) std::copy(offdiag, offdiag + E * 36, st + N * 42);
    if (Es) { std::copy(sw_c, sw_c + Es * 12, st + N * 42 + E * 36); std::copy(sw_hss, sw_hss + Es, st + N * 42 + E * 36 + Es * 12); std::copy(sw_gs, sw_gs + Es, st + N * 42 + E * 36 + Es * 13); }
    const int nc = c.nc();
    const ScLmView& V = lm->V;
    double* w = c.vec.as<double>();
    double* x = w + 2 * (size_t)nc;
    double* dp = lm->out.as<double>();
    double* ds = dp + N * 6;
    double* d3 = ds + Es;
    SCHIP(c.err, hipEventRecord(lm->ev[0], c.st));
    SCHIP(c.err, hipMemcpyAsync(lm->num.p, st, lm->stage.size() * sizeof(double), hipMemcpyHostToDevice, c.st));
    SCHIP(c.err, hipEventRecord(lm->ev[1], c.st));
    SCHIP(c.err, hipMemsetAsync(c.fail.p, 0, sizeof(int32_t), c.st));
    SCHIP(c.err, hipMemsetAsync(c.T.p, 0, (size_t)c.P.tiles() * SC_TILE * sizeof(double), c.st));
    hipLaunchKernelGGL(sc_lm_scale_kernel, sc_grid((int64_t)(N * 6 + Es)), dim3(SC_THREADS), 0, c.st, V, radius, min_lm_diagonal, max_lm_diagonal, c.fail.as<int32_t>());
    hipLaunchKernelGGL(sc_lm_fill_kernel, sc_grid(sc_lm_fill_threads(V)), dim3(SC_THREADS), 0, c.st, c.T.as<double>(), c.D, V);
    hipLaunchKernelGGL(sc_lm_rhs_kernel, sc_grid(nc), dim3(SC_THREADS), 0, c.st, V, w);
    SCHIP(c.err, hipEventRecord(lm->ev[2], c.st));
    ScLaunch Ln = c.launcher(1, w, w + nc, x, 0, true);
    sc_factor_steps(c.P, Ln);
    SCHIP(c.err, hipEventRecord(lm->ev[3], c.st));
    sc_solve_steps(c.P, Ln);      // (a failed factor: the sweeps and what follows run on numbers nobody reads — every address comes from the plan, none from the numbers)
    SCHIP(c.err, hipEventRecord(lm->ev[4], c.st));
    hipLaunchKernelGGL(sc_lm_backsub_kernel, sc_grid((int64_t)(N * 6 + Es)), dim3(SC_THREADS), 0, c.st, V, (const double*)x, dp, ds);
    hipLaunchKernelGGL(sc_lm_model_kernel, dim3((unsigned)lm->blocks()), dim3(SC_THREADS), 0, c.st, V, (const double*)dp, (const double*)ds, lm->part.as<double>());
    hipLaunchKernelGGL(sc_lm_reduce_kernel, dim3(1), dim3(64), 0, c.st, lm->part.as<const double>(), lm->blocks(), d3);
    SCHIP(c.err, hipEventRecord(lm->ev[5], c.st));
    SCHIP(c.err, hipMemcpyAsync(lm->h_out.data(), lm->out.p, lm->h_out.size() * sizeof(double), hipMemcpyDeviceToHost, c.st));
    SCHIP(c.err, hipEventRecord(lm->ev[6], c.st));
    int32_t fail = 1;
    SCHIP(c.err, hipMemcpyAsync(&fail, c.fail.p, sizeof(fail), hipMemcpyDeviceToHost, c.st));
    SCHIP(c.err, hipStreamSynchronize(c.st));
    SCHIP(c.err, hipGetLastError());
    for (int k = 0; k < 6; ++k) { float ms = 0; SCHIP(c.err, hipEventElapsedTime(&ms, lm->ev[k], lm->ev[k + 1])); lm->ms[k] = ms; }
    c.last_ms = lm->ms[2];
    out3[2] = lm->ms[2];
    if (fail) { c.err = "pgo_sparse_lm_step: a pivot of the damped system is not > 0"; return PGO_ERR_NUMERIC; }
    std::copy(lm->h_out.begin(), lm->h_out.begin() + (std::ptrdiff_t)(N * 6), delta_pose);
    if (Es) std::copy(lm->h_out.begin() + (std::ptrdiff_t)(N * 6), lm->h_out.begin() + (std::ptrdiff_t)(N * 6 + Es), delta_sw);
    out3[0] = lm->h_out[N * 6 + Es]; out3[1] = lm->h_out[N * 6 + Es + 1];
    return PGO_OK;
}

int pgo_sparse_lm_last_times(const pgo_sparse_lm* lm, double* ms6) {
    if (!lm || !ms6) return PGO_ERR_INVALID_ARG;
    std::copy(lm->ms, lm->ms + 6, ms6);
    return PGO_OK;
}

int pgo_sparse_lm_solve(pgo_sparse_lm* lm, const pgo_sparse_lm_callbacks* cb, void* user, int64_t n_switch, const int32_t* swe_index, double* quat, double* t, double* sw, const pgo_options* opts,
                        pgo_summary* summary) {
    if (!lm) return PGO_ERR_INVALID_ARG;
    ScCore& c = lm->chol->c;
    c.err.clear();
    if (!cb || !cb->evaluate || !cb->normal_blocks || !cb->manifold_plus || !quat || !t || !opts || n_switch < 0 || (n_switch > 0 && !sw) || (lm->plan.n_sw > 0 && n_switch < 1)) {
        c.err = "pgo_sparse_lm_solve: null pointer, or switchable edges without switches"; return PGO_ERR_INVALID_ARG;
    }
    ScLmDeviceStepper S{lm};
    const ScLmCallbacks k{cb->evaluate, cb->normal_blocks, cb->manifold_plus};
    const int rc = sc_lm_solve(S, lm->plan, k, user, n_switch, swe_index, quat, t, sw, *opts, summary);
    if (rc != PGO_OK && c.err.empty()) c.err = rc == PGO_ERR_INVALID_ARG ? "pgo_sparse_lm_solve: a switch index is out of range, or a callback refused its arguments" : "pgo_sparse_lm_solve: a callback failed";
    return rc;
}

}  // extern "C"
