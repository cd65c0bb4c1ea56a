// pgo_sparse.hip — libpgo_sparse.so (include/pgo_sparse.h): the tile-sparse exact Cholesky solver on the device, host side and C entry points.  The kernels are in
// pgo_sparse_kernels.hpp (what they share: pgo_tile_ops.hpp); the exact LM step and solve on this factor (pgo_sparse_lm_*) in pgo_sparse_lm.hpp, the self-linearising graph (pgo_sparse_graph_*) in pgo_sparse_graph.hpp and the 4-DoF graph (pgo_sparse_yaw_graph_*) in pgo_sparse_yaw.hpp, all three included at the end of this file: one translation unit.
// This library neither links nor changes libpgo.so.
//
// The step order is sc_factor_steps / sc_solve_steps / sc_selinv_steps / sc_panel_steps (pgo_sparse_math.hpp), nowhere else: the structs ScLaunch, ScSelLaunch and
// ScPanelLaunch below turn a step into its launch.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>

#include "pgo_sparse.h"
#include "pgo_sparse_kernels.hpp"

namespace pgo {

namespace {

// ---- host side
thread_local std::string g_err;    // the last error of a call without an object

// a device buffer.  It enters its owner's list where it is declared — it cannot be declared without — and the owner releases its list: no second list of names.  The
// list holds pointers to the owner's members: neither a DevBuf nor, with it, its owner can be copied or moved
struct DevBuf;
using DevBufs = std::vector<DevBuf*>;
struct DevBuf {
    void* p = nullptr; size_t bytes = 0;
    explicit DevBuf(DevBufs& owner) { owner.push_back(this); }
    DevBuf(const DevBuf&) = delete;
    DevBuf(DevBuf&&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf& operator=(DevBuf&&) = delete;
    hipError_t ensure(size_t b) {
        if (b <= bytes && p) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr; bytes = 0;
        const hipError_t e = hipMalloc(&p, b ? b : 8);
        if (e == hipSuccess) bytes = b ? b : 8; else p = nullptr;
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
    template <class V> V* as() const { return static_cast<V*>(p); }
};
void release_all(const DevBufs& bufs) { for (DevBuf* b : bufs) b->release(); }

// the 1-D grid of one thread per item
dim3 sc_grid(int64_t items) { return dim3((unsigned)((items + SC_THREADS - 1) / SC_THREADS)); }

#define SCHIP(err, call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) { (err) = std::string(#call) + ": " + hipGetErrorString(e_); return e_ == hipErrorOutOfMemory ? PGO_ERR_OUT_OF_MEMORY : PGO_ERR_HIP; } } while (0)

// the launches, walked by sc_factor_steps and sc_solve_steps.  first_forward: the forward steps before it are skipped (they would solve and subtract +0); with_backward
// = false: the forward sweep alone
struct ScLaunch {
    double* T; ScDev D; const ScPlan* P; double* LT; int32_t* fail; int nc; unsigned n_rhs; double* w; double* yv; double* x; int first_forward; bool with_backward; hipStream_t st;
    void factor_diag(int k, bool) { hipLaunchKernelGGL(sc_diag_kernel, dim3(1), dim3(SC_THREADS), 0, st, T, P->diag(k), fail); }
    void panel(int k) { hipLaunchKernelGGL(sc_panel_kernel, dim3((unsigned)P->s_size(k)), dim3(SC_THREADS), 0, st, T, D, k, P->ldu(), LT); }
    void update(int k) { const unsigned m = (unsigned)P->s_size(k); hipLaunchKernelGGL(sc_update_kernel, dim3(m * (m + 1) / 2), dim3(SC_THREADS), 0, st, T, D, k, P->ldu(), (const double*)LT, fail); }
    void forward(int k) { if (k >= first_forward) hipLaunchKernelGGL(sc_forward_kernel, dim3((unsigned)(1 + P->s_size(k)), n_rhs), dim3(SC_THREADS), 0, st, (const double*)T, D, k, nc, w, yv); }
    void backward(int k) {
        if (with_backward) hipLaunchKernelGGL(sc_backward_kernel, dim3((unsigned)(P->row_ptr[(size_t)k + 1] - P->row_ptr[(size_t)k]), n_rhs), dim3(SC_THREADS), 0, st, (const double*)T, D, k, nc, yv, x);
    }
};

// the launches of the selected inverse, walked by sc_selinv_steps.  G: the panel scratch (ScPlan::scratch_doubles() holds max |s_k| tiles)
struct ScSelLaunch {
    const double* T; double* Z; ScDev D; const ScPlan* P; double* G; hipStream_t st;
    void ginv(int k) { hipLaunchKernelGGL(sc_sel_ginv_kernel, dim3((unsigned)P->s_size(k)), dim3(SC_THREADS), 0, st, T, D, k, G); }
    void column(int k) { hipLaunchKernelGGL(sc_sel_column_kernel, dim3((unsigned)P->s_size(k)), dim3(SC_THREADS), 0, st, Z, D, k, (const double*)G); }
    void diag(int k) { hipLaunchKernelGGL(sc_sel_diag_kernel, dim3(1), dim3(SC_THREADS), 0, st, Z, D, k, (const double*)G); }
    void inverses() { hipLaunchKernelGGL(sc_sel_inverses_kernel, dim3((unsigned)P->nt), dim3(SC_THREADS), 0, st, T, Z, D); }
};

// the launches of the panel sweeps, walked by sc_panel_steps
struct ScPanelLaunch {
    const double* T; ScDev D; int nc; double* W; const int32_t* first; hipStream_t st;
    void pfwd(int k, int started) { hipLaunchKernelGGL(sc_pfwd_kernel, dim3((unsigned)started), dim3(SC_THREADS), 0, st, T, D, k, nc, W, first); }
    void pbwd(int k, int panels) { hipLaunchKernelGGL(sc_pbwd_kernel, dim3((unsigned)panels), dim3(SC_THREADS), 0, st, T, D, k, nc, W); }
};

// a device, a stream, a plan with its tables, tile storage and panel scratch
struct ScCore {
    int device = -1; hipStream_t st = nullptr; hipEvent_t e0 = nullptr, e1 = nullptr;
    ScPlan P; ScDev D{};
    DevBufs bufs;
    DevBuf tables{bufs}, T{bufs}, LT{bufs}, vec{bufs}, fail{bufs};
    std::string err;
    double last_ms = 0.0;
    int nc() const { return P.nt * DC_NB; }
    int open(int device_id) {
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess || count < 1) { err = "no HIP device"; return PGO_ERR_NO_DEVICE; }
        if (device_id == -1 && hipGetDevice(&device_id) != hipSuccess) { err = "no current HIP device"; return PGO_ERR_NO_DEVICE; }      // (pgo_options.device_id's convention)
        if (device_id < 0 || device_id >= count) { err = "no such HIP device"; return PGO_ERR_NO_DEVICE; }
        SCHIP(err, hipSetDevice(device_id));
        device = device_id;
        SCHIP(err, hipStreamCreate(&st));
        SCHIP(err, hipEventCreate(&e0)); SCHIP(err, hipEventCreate(&e1));
        return PGO_OK;
    }
    int use() { SCHIP(err, hipSetDevice(device)); return PGO_OK; }
    // the plan's six tables as int32, one upload; tile storage, scratch, failure flag
    int upload_plan() {
        std::vector<int32_t> h;
        size_t at[6];
        const std::vector<int32_t> ahead(P.ahead.begin(), P.ahead.end());
        const std::vector<int32_t>* parts[6] = {&P.row_ptr, &P.row_col, &P.col_ptr, &P.col_row, &P.col_tile, &ahead};
        for (int k = 0; k < 6; ++k) { at[k] = h.size(); h.insert(h.end(), parts[k]->begin(), parts[k]->end()); }
        SCHIP(err, tables.ensure(h.size() * sizeof(int32_t)));
        SCHIP(err, hipMemcpy(tables.p, h.data(), h.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        const int32_t* d = tables.as<int32_t>();
        D = ScDev{d + at[0], d + at[1], d + at[2], d + at[3], d + at[4], d + at[5]};
        SCHIP(err, T.ensure((size_t)P.tiles() * SC_TILE * sizeof(double)));
        SCHIP(err, LT.ensure(P.scratch_doubles() * sizeof(double)));
        SCHIP(err, fail.ensure(sizeof(int32_t)));
        return PGO_OK;
    }
    ScLaunch launcher(unsigned n_rhs, double* w, double* yv, double* x, int first_forward, bool with_backward) {
        return ScLaunch{T.as<double>(), D, &P, LT.as<double>(), fail.as<int32_t>(), nc(), n_rhs, w, yv, x, first_forward, with_backward, st};
    }
    // after a run of launches between e0 and e1: the stream's end, the launches' errors, the events' time
    int finish() {
        SCHIP(err, hipStreamSynchronize(st));
        SCHIP(err, hipGetLastError());
        float ms = 0;
        SCHIP(err, hipEventElapsedTime(&ms, e0, e1));
        last_ms = ms;
        return PGO_OK;
    }
    void close() {
        if (device < 0) return;
        (void)hipSetDevice(device);
        if (st) (void)hipStreamSynchronize(st);
        release_all(bufs);
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        if (st) (void)hipStreamDestroy(st);
        st = nullptr; e0 = e1 = nullptr; device = -1;
    }
};

void plan_info(const ScPlan& P, int used, int64_t* info8) {
    const int64_t v[8] = {P.nt, P.a_tiles, P.tiles(), used, (int64_t)(P.tiles() * (int64_t)SC_TILE * 8), P.factor_launches(), P.solve_launches(), P.tile_updates()};
    std::copy(v, v + 8, info8);
}

}  // namespace

}  // namespace pgo

using namespace pgo;

struct pgo_sparse_chol {
    ScCore c;
    int64_t N = 0, n_pairs = 0;
    DevBufs bufs;                                          // of the DevBuf members below
    int used = 0;
    bool factored = false;
    bool selected = false;      // Z holds the selected inverse of the present factor
    std::vector<uint8_t> in_system;
    std::vector<int32_t> order, pos;
    std::vector<int32_t> h_hi, h_lo;                       // the pair list as pgo_sparse_chol_create took it (pgo_sparse_lm_create reads it)
    DevBuf d_in{bufs}, d_pos{bufs}, d_hi{bufs}, d_lo{bufs}, d_diag{bufs}, d_blocks{bufs}, d_at{bufs}, d_val{bufs}, d_pr{bufs}, d_out{bufs}, Z{bufs}, d_na{bufs}, d_nb{bufs}, d_flag{bufs};
    DevBuf ws{bufs}, d_req{bufs};                      // pgo_sparse_chol_inverse_columns: W of one chunk, the chunk's tables
    int64_t ws_limit = PGO_SPARSE_WORKSPACE_BYTES;
    int64_t cols_info[4] = {0, 0, 0, 0};                   // of the last pgo_sparse_chol_inverse_columns
    void release() {
        if (c.device >= 0) (void)hipSetDevice(c.device);
        if (c.st) (void)hipStreamSynchronize(c.st);
        release_all(bufs);
        c.close();
    }
};

// the tail of inverse_blocks, selected_blocks and inverse_columns: the end of the timed launches, the nb 36-double blocks of d_out (and the nb flags of d_flag) to the
// host, the stream's end.  The caller copies out what it then decides to return.
static int download_blocks(pgo_sparse_chol* h, size_t nb, std::vector<double>& blocks, std::vector<uint8_t>* flags) {
    ScCore& c = h->c;
    SCHIP(c.err, hipEventRecord(c.e1, c.st));
    blocks.resize(nb * 36);
    SCHIP(c.err, hipMemcpyAsync(blocks.data(), h->d_out.p, blocks.size() * sizeof(double), hipMemcpyDeviceToHost, c.st));
    if (flags) { std::vector<uint8_t>& flag = *flags; flag.resize(nb); SCHIP(c.err, hipMemcpyAsync(flag.data(), h->d_flag.p, nb, hipMemcpyDeviceToHost, c.st)); }
    return c.finish();
}

extern "C" {

const char* pgo_sparse_strerror(int code) {
    switch (code) {
        case PGO_OK: return "ok";
        case PGO_ERR_INVALID_ARG: return "invalid argument";
        case PGO_ERR_NO_DEVICE: return "no HIP device";
        case PGO_ERR_HIP: return "a HIP call failed";
        case PGO_ERR_OUT_OF_MEMORY: return "out of device memory";
        case PGO_ERR_STATE: return "call order violated";
        case PGO_ERR_NUMERIC: return "the matrix is not numerically positive definite";
        default: return "unknown error";
    }
}
const char* pgo_sparse_last_error(const pgo_sparse_chol* h) { return h ? h->c.err.c_str() : g_err.c_str(); }

int pgo_sparse_spd_solve(int32_t device_id, int32_t n, const double* a, const double* b, const int32_t* pos, double* x, int64_t* info8, int32_t launches, double* avg_ms) {
    g_err.clear();
    if (n <= 0 || n > (1 << 30) || !a || !b || !x || launches < 1) { g_err = "pgo_sparse_spd_solve: null pointer, n <= 0 or launches < 1"; return PGO_ERR_INVALID_ARG; }
    if (pos) {
        std::vector<uint8_t> seen((size_t)n, 0);
        for (int i = 0; i < n; ++i) { if (pos[i] < 0 || pos[i] >= n || seen[(size_t)pos[i]]) { g_err = "pgo_sparse_spd_solve: pos is not a permutation of 0 .. n - 1"; return PGO_ERR_INVALID_ARG; } seen[(size_t)pos[i]] = 1; }
    }
    ScCore c;
    struct Closer { ScCore& c; ~Closer() { g_err = c.err; c.close(); } } closer{c};
    int rc;
    if ((rc = c.open(device_id)) != PGO_OK) return rc;
    c.P = sc_plan_matrix(n, a, pos);
    if (info8) plan_info(c.P, 0, info8);
    if ((rc = c.upload_plan()) != PGO_OK) return rc;
    const int nc = c.nc();
    std::vector<double> hT((size_t)c.P.tiles() * SC_TILE, 0.0), hw((size_t)nc, 0.0);
    sc_fill_tiles(c.P, n, a, pos, hT.data());
    for (int i = 0; i < n; ++i) hw[(size_t)(pos ? pos[i] : i)] = b[i];
    SCHIP(c.err, c.vec.ensure((size_t)3 * nc * sizeof(double)));
    double* w = c.vec.as<double>();
    ScLaunch L = c.launcher(1, w, w + nc, w + 2 * (size_t)nc, 0, true);
    double total = 0.0;
    int32_t fail = 0;
    for (int l = 0; l < launches && !fail; ++l) {
        SCHIP(c.err, hipMemcpyAsync(c.T.p, hT.data(), hT.size() * sizeof(double), hipMemcpyHostToDevice, c.st));
        SCHIP(c.err, hipMemcpyAsync(w, hw.data(), hw.size() * sizeof(double), hipMemcpyHostToDevice, c.st));
        SCHIP(c.err, hipMemsetAsync(c.fail.p, 0, sizeof(int32_t), c.st));
        SCHIP(c.err, hipEventRecord(c.e0, c.st));
        sc_factor_steps(c.P, L);
        sc_solve_steps(c.P, L);      // (a failed factor: the sweeps run on numbers nobody reads — every address comes from the plan, none from the numbers)
        SCHIP(c.err, hipEventRecord(c.e1, c.st));
        SCHIP(c.err, hipMemcpyAsync(&fail, c.fail.p, sizeof(fail), hipMemcpyDeviceToHost, c.st));
        if ((rc = c.finish()) != PGO_OK) return rc;
        total += c.last_ms;
    }
    if (avg_ms) *avg_ms = total / launches;
    if (fail) { c.err = "pgo_sparse_spd_solve: the matrix is not numerically positive definite"; return PGO_ERR_NUMERIC; }
    SCHIP(c.err, hipMemcpy(hw.data(), w + 2 * (size_t)nc, hw.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) x[i] = hw[(size_t)(pos ? pos[i] : i)];
    return PGO_OK;
}

int pgo_sparse_chol_create(int32_t device_id, int64_t n_nodes, const uint8_t* in_system, int64_t n_pairs, const int32_t* pair_hi, const int32_t* pair_lo, int32_t ordering, pgo_sparse_chol** out) {
    g_err.clear();
    if (!out) { g_err = "pgo_sparse_chol_create: null pointer"; return PGO_ERR_INVALID_ARG; }
    *out = nullptr;
    if (n_nodes < 1 || n_nodes > (int64_t)300000000 || !in_system || n_pairs < 0 || (n_pairs > 0 && (!pair_hi || !pair_lo)) || ordering < -1 || ordering > 1) {
        g_err = "pgo_sparse_chol_create: null pointer, count out of range or unknown ordering"; return PGO_ERR_INVALID_ARG;
    }
    if (const char* what = sc_check_pairs(n_nodes, in_system, n_pairs, pair_hi, pair_lo)) { g_err = std::string("pgo_sparse_chol_create: ") + what; return PGO_ERR_INVALID_ARG; }
    pgo_sparse_chol* h = new pgo_sparse_chol;
    struct Guard { pgo_sparse_chol* h; ~Guard() { if (h) { g_err = h->c.err; h->release(); delete h; } } } guard{h};
    int rc;
    if ((rc = h->c.open(device_id)) != PGO_OK) return rc;
    h->N = n_nodes; h->n_pairs = n_pairs;
    h->in_system.assign(in_system, in_system + n_nodes);
    if (n_pairs) { h->h_hi.assign(pair_hi, pair_hi + n_pairs); h->h_lo.assign(pair_lo, pair_lo + n_pairs); }
    std::vector<int64_t> adj_ptr; std::vector<int32_t> adj;
    sc_pair_adjacency(n_nodes, n_pairs, pair_hi, pair_lo, adj_ptr, adj);
    h->c.P = sc_plan_graph(n_nodes, adj_ptr.data(), adj.data(), in_system, ordering, h->order, &h->used);
    h->pos.assign((size_t)n_nodes, 0);
    for (int64_t q = 0; q < n_nodes; ++q) h->pos[(size_t)h->order[(size_t)q]] = (int32_t)q;
    if ((rc = h->c.upload_plan()) != PGO_OK) return rc;
    ScCore& c = h->c;
    SCHIP(c.err, h->d_in.ensure((size_t)n_nodes)); SCHIP(c.err, h->d_pos.ensure((size_t)n_nodes * sizeof(int32_t)));
    SCHIP(c.err, h->d_hi.ensure((size_t)n_pairs * sizeof(int32_t))); SCHIP(c.err, h->d_lo.ensure((size_t)n_pairs * sizeof(int32_t)));
    SCHIP(c.err, h->d_diag.ensure((size_t)n_nodes * 36 * sizeof(double))); SCHIP(c.err, h->d_blocks.ensure((size_t)n_pairs * 36 * sizeof(double)));
    SCHIP(c.err, hipMemcpy(h->d_in.p, in_system, (size_t)n_nodes, hipMemcpyHostToDevice));
    SCHIP(c.err, hipMemcpy(h->d_pos.p, h->pos.data(), (size_t)n_nodes * sizeof(int32_t), hipMemcpyHostToDevice));
    if (n_pairs) {
        SCHIP(c.err, hipMemcpy(h->d_hi.p, pair_hi, (size_t)n_pairs * sizeof(int32_t), hipMemcpyHostToDevice));
        SCHIP(c.err, hipMemcpy(h->d_lo.p, pair_lo, (size_t)n_pairs * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    guard.h = nullptr;
    *out = h;
    return PGO_OK;
}

void pgo_sparse_chol_destroy(pgo_sparse_chol* h) {
    if (!h) return;
    h->release();
    delete h;
}

int pgo_sparse_chol_info(const pgo_sparse_chol* h, int64_t* info8, int32_t* order) {
    if (!h) return PGO_ERR_INVALID_ARG;
    if (info8) plan_info(h->c.P, h->used, info8);
    if (order) std::copy(h->order.begin(), h->order.end(), order);
    return PGO_OK;
}

double pgo_sparse_chol_last_ms(const pgo_sparse_chol* h) { return h ? h->c.last_ms : 0.0; }

int pgo_sparse_chol_factor(pgo_sparse_chol* h, const double* diag, const double* pair_blocks) {
    if (!h) return PGO_ERR_INVALID_ARG;
    ScCore& c = h->c;
    c.err.clear();
    if (!diag || (h->n_pairs > 0 && !pair_blocks)) { c.err = "pgo_sparse_chol_factor: null pointer"; return PGO_ERR_INVALID_ARG; }
    int rc;
    if ((rc = c.use()) != PGO_OK) return rc;
    h->factored = false;
    h->selected = false;      // (Z, if there is one, belongs to the factor before)
    const int nc = c.nc();
    SCHIP(c.err, hipMemcpyAsync(h->d_diag.p, diag, (size_t)h->N * 36 * sizeof(double), hipMemcpyHostToDevice, c.st));
    if (h->n_pairs) SCHIP(c.err, hipMemcpyAsync(h->d_blocks.p, pair_blocks, (size_t)h->n_pairs * 36 * sizeof(double), hipMemcpyHostToDevice, c.st));
    SCHIP(c.err, hipMemsetAsync(c.fail.p, 0, sizeof(int32_t), c.st));
    SCHIP(c.err, hipEventRecord(c.e0, c.st));
    SCHIP(c.err, hipMemsetAsync(c.T.p, 0, (size_t)c.P.tiles() * SC_TILE * sizeof(double), c.st));
    const int64_t threads = h->N * 36 + ((int64_t)nc - h->N * 6) + h->n_pairs * 36;
    hipLaunchKernelGGL(sc_fill_kernel, sc_grid(threads), dim3(SC_THREADS), 0, c.st, c.T.as<double>(), c.D, h->N, nc, h->d_in.as<const uint8_t>(),
                       h->d_pos.as<const int32_t>(), h->d_diag.as<const double>(), h->n_pairs, h->d_hi.as<const int32_t>(), h->d_lo.as<const int32_t>(), h->d_blocks.as<const double>());
    ScLaunch L = c.launcher(1, nullptr, nullptr, nullptr, 0, false);
    sc_factor_steps(c.P, L);
    SCHIP(c.err, hipEventRecord(c.e1, c.st));
    int32_t fail = 1;
    SCHIP(c.err, hipMemcpyAsync(&fail, c.fail.p, sizeof(fail), hipMemcpyDeviceToHost, c.st));
    if ((rc = c.finish()) != PGO_OK) return rc;
    if (fail) { c.err = "pgo_sparse_chol_factor: the matrix is not numerically positive definite"; return PGO_ERR_NUMERIC; }
    h->factored = true;
    return PGO_OK;
}

int pgo_sparse_chol_solve(pgo_sparse_chol* h, int64_t n_rhs, const double* B, double* X) {
    if (!h) return PGO_ERR_INVALID_ARG;
    ScCore& c = h->c;
    c.err.clear();
    if (n_rhs < 1 || n_rhs > PGO_SPARSE_MAX_RHS || !B || !X) { c.err = "pgo_sparse_chol_solve: null pointer, or n_rhs outside 1 .. PGO_SPARSE_MAX_RHS"; return PGO_ERR_INVALID_ARG; }
    if (!h->factored) { c.err = "pgo_sparse_chol_solve: no factor (pgo_sparse_chol_factor has not succeeded)"; return PGO_ERR_STATE; }
    int rc;
    if ((rc = c.use()) != PGO_OK) return rc;
    const size_t nc = (size_t)c.nc(), n6 = (size_t)h->N * 6, total = (size_t)n_rhs * nc;
    std::vector<double> hw(total, 0.0);
    for (int64_t r = 0; r < n_rhs; ++r)
        for (int64_t i = 0; i < h->N; ++i)
            if (h->in_system[(size_t)i]) std::memcpy(&hw[(size_t)r * nc + (size_t)h->pos[(size_t)i] * 6], B + (size_t)r * n6 + (size_t)i * 6, 6 * sizeof(double));
    SCHIP(c.err, c.vec.ensure(3 * total * sizeof(double)));
    double* w = c.vec.as<double>();
    SCHIP(c.err, hipMemcpyAsync(w, hw.data(), total * sizeof(double), hipMemcpyHostToDevice, c.st));
    ScLaunch L = c.launcher((unsigned)n_rhs, w, w + total, w + 2 * total, 0, true);
    SCHIP(c.err, hipEventRecord(c.e0, c.st));
    sc_solve_steps(c.P, L);
    SCHIP(c.err, hipEventRecord(c.e1, c.st));
    SCHIP(c.err, hipMemcpyAsync(hw.data(), w + 2 * total, total * sizeof(double), hipMemcpyDeviceToHost, c.st));
    if ((rc = c.finish()) != PGO_OK) return rc;
    for (int64_t r = 0; r < n_rhs; ++r)
        for (int64_t i = 0; i < h->N; ++i) {
            double* xo = X + (size_t)r * n6 + (size_t)i * 6;
            if (h->in_system[(size_t)i]) std::memcpy(xo, &hw[(size_t)r * nc + (size_t)h->pos[(size_t)i] * 6], 6 * sizeof(double));
            else std::fill(xo, xo + 6, 0.0);
        }
    return PGO_OK;
}

int pgo_sparse_chol_inverse_blocks(pgo_sparse_chol* h, int64_t n_groups, const int64_t* group_ptr, const int64_t* row_ptr, const int32_t* col, const double* val,
                                   int64_t n_pairs, const int32_t* ga, const int32_t* gb, double* out) {
    if (!h) return PGO_ERR_INVALID_ARG;
    ScCore& c = h->c;
    c.err.clear();
    if (n_groups < 1 || n_groups > PGO_SPARSE_MAX_GROUPS) { c.err = "pgo_sparse_chol_inverse_blocks: the number of groups is outside 1 .. PGO_SPARSE_MAX_GROUPS"; return PGO_ERR_INVALID_ARG; }
    if (!group_ptr || !row_ptr || n_pairs < 0 || (n_pairs > 0 && (!ga || !gb || !out))) { c.err = "pgo_sparse_chol_inverse_blocks: null pointer or negative count"; return PGO_ERR_INVALID_ARG; }
    for (int64_t k = 0; k < n_pairs; ++k) if (ga[k] < 0 || ga[k] >= n_groups || gb[k] < 0 || gb[k] >= n_groups) { c.err = "pgo_sparse_chol_inverse_blocks: a pair names a group out of range"; return PGO_ERR_INVALID_ARG; }
    if (!h->factored) { c.err = "pgo_sparse_chol_inverse_blocks: no factor (pgo_sparse_chol_factor has not succeeded)"; return PGO_ERR_STATE; }
    const int nc = c.nc();
    const ScRows R(h->N, h->in_system.data(), h->pos.data(), nc, n_groups, group_ptr, row_ptr, col, val);
    if (R.error) { c.err = std::string("pgo_sparse_chol_inverse_blocks: ") + R.error; return PGO_ERR_INVALID_ARG; }
    if (n_pairs == 0) return PGO_OK;
    int rc;
    if ((rc = c.use()) != PGO_OK) return rc;
    const size_t total = (size_t)R.rows * nc, nnz = R.at.size();
    std::vector<int32_t> pr;
    for (int64_t k = 0; k < n_pairs; ++k) for (int32_t v : {R.first_row[(size_t)ga[k]], R.first_row[(size_t)gb[k]], R.dim[(size_t)ga[k]] | (R.dim[(size_t)gb[k]] << 8)}) pr.push_back(v);
    SCHIP(c.err, c.vec.ensure(2 * total * sizeof(double)));
    SCHIP(c.err, h->d_at.ensure(nnz * sizeof(int64_t))); SCHIP(c.err, h->d_val.ensure(nnz * sizeof(double)));
    SCHIP(c.err, h->d_pr.ensure(pr.size() * sizeof(int32_t))); SCHIP(c.err, h->d_out.ensure((size_t)n_pairs * 36 * sizeof(double)));
    double* w = c.vec.as<double>();
    double* yv = w + total;
    if (nnz) {
        SCHIP(c.err, hipMemcpyAsync(h->d_at.p, R.at.data(), nnz * sizeof(int64_t), hipMemcpyHostToDevice, c.st));
        SCHIP(c.err, hipMemcpyAsync(h->d_val.p, R.val.data(), nnz * sizeof(double), hipMemcpyHostToDevice, c.st));
    }
    SCHIP(c.err, hipMemcpyAsync(h->d_pr.p, pr.data(), pr.size() * sizeof(int32_t), hipMemcpyHostToDevice, c.st));
    SCHIP(c.err, hipEventRecord(c.e0, c.st));
    SCHIP(c.err, hipMemsetAsync(w, 0, 2 * total * sizeof(double), c.st));      // (y of the skipped steps: the zeros the Gram products read as such)
    if (nnz) hipLaunchKernelGGL(sc_rhs_kernel, sc_grid((int64_t)nnz), dim3(SC_THREADS), 0, c.st, w, (int64_t)nnz, h->d_at.as<const int64_t>(), h->d_val.as<const double>());
    ScLaunch L = c.launcher((unsigned)R.rows, w, yv, nullptr, R.first_tile, false);
    sc_solve_steps(c.P, L);
    const int c0 = std::min(R.first_tile * DC_NB, nc) / DC_GRAM * DC_GRAM;      // every column before it holds zeros in every row
    hipLaunchKernelGGL(sc_gram_kernel, dim3((unsigned)n_pairs), dim3(SC_THREADS), 0, c.st, (const double*)yv, nc, c0, h->d_pr.as<const int32_t>(), h->d_out.as<double>());
    std::vector<double> blocks;
    if ((rc = download_blocks(h, (size_t)n_pairs, blocks, nullptr)) != PGO_OK) return rc;
    std::copy(blocks.begin(), blocks.end(), out);
    return PGO_OK;
}

int pgo_sparse_chol_selected_inverse(pgo_sparse_chol* h) {
    if (!h) return PGO_ERR_INVALID_ARG;
    ScCore& c = h->c;
    c.err.clear();
    if (!h->factored) { c.err = "pgo_sparse_chol_selected_inverse: no factor (pgo_sparse_chol_factor has not succeeded)"; return PGO_ERR_STATE; }
    int rc;
    if ((rc = c.use()) != PGO_OK) return rc;
    h->selected = false;
    SCHIP(c.err, h->Z.ensure((size_t)c.P.tiles() * SC_TILE * sizeof(double)));      // (every tile is written by the step of its column: no memset)
    ScSelLaunch L{c.T.as<const double>(), h->Z.as<double>(), c.D, &c.P, c.LT.as<double>(), c.st};
    SCHIP(c.err, hipEventRecord(c.e0, c.st));
    sc_selinv_steps(c.P, L);
    SCHIP(c.err, hipEventRecord(c.e1, c.st));
    if ((rc = c.finish()) != PGO_OK) return rc;
    h->selected = true;
    return PGO_OK;
}

int pgo_sparse_chol_selected_info(const pgo_sparse_chol* h, int64_t* info4) {
    if (!h || !info4) return PGO_ERR_INVALID_ARG;
    const ScPlan& P = h->c.P;
    const int64_t v[4] = {P.selinv_launches(), P.selinv_products(), (int64_t)(P.tiles() * (int64_t)SC_TILE * 8), h->selected ? 1 : 0};
    std::copy(v, v + 4, info4);
    return PGO_OK;
}

int pgo_sparse_chol_selected_blocks(pgo_sparse_chol* h, int64_t n_blocks, const int32_t* node_a, const int32_t* node_b, double* out, uint8_t* in_pattern) {
    if (!h) return PGO_ERR_INVALID_ARG;
    ScCore& c = h->c;
    c.err.clear();
    if (n_blocks < 0 || n_blocks > (int64_t)50000000 || (n_blocks > 0 && (!node_a || !node_b || !out))) { c.err = "pgo_sparse_chol_selected_blocks: null pointer or count out of range"; return PGO_ERR_INVALID_ARG; }
    for (int64_t k = 0; k < n_blocks; ++k)
        if (node_a[k] < 0 || node_a[k] >= h->N || node_b[k] < 0 || node_b[k] >= h->N) { c.err = "pgo_sparse_chol_selected_blocks: block " + std::to_string(k) + " names a keyframe out of range"; return PGO_ERR_INVALID_ARG; }
    if (!h->selected) { c.err = "pgo_sparse_chol_selected_blocks: no selected inverse of the present factor (pgo_sparse_chol_selected_inverse has not succeeded since the last pgo_sparse_chol_factor)"; return PGO_ERR_STATE; }
    if (n_blocks == 0) return PGO_OK;
    int rc;
    if ((rc = c.use()) != PGO_OK) return rc;
    const size_t nb = (size_t)n_blocks;
    SCHIP(c.err, h->d_na.ensure(nb * sizeof(int32_t))); SCHIP(c.err, h->d_nb.ensure(nb * sizeof(int32_t)));
    SCHIP(c.err, h->d_out.ensure(nb * 36 * sizeof(double))); SCHIP(c.err, h->d_flag.ensure(nb));
    SCHIP(c.err, hipMemcpyAsync(h->d_na.p, node_a, nb * sizeof(int32_t), hipMemcpyHostToDevice, c.st));
    SCHIP(c.err, hipMemcpyAsync(h->d_nb.p, node_b, nb * sizeof(int32_t), hipMemcpyHostToDevice, c.st));
    SCHIP(c.err, hipEventRecord(c.e0, c.st));
    hipLaunchKernelGGL(sc_sel_gather_kernel, sc_grid((int64_t)nb * 36), dim3(SC_THREADS), 0, c.st, h->Z.as<const double>(), c.D, n_blocks, h->d_na.as<const int32_t>(),
                       h->d_nb.as<const int32_t>(), h->d_in.as<const uint8_t>(), h->d_pos.as<const int32_t>(), h->d_out.as<double>(), h->d_flag.as<uint8_t>());
    std::vector<double> blocks;
    std::vector<uint8_t> flag;
    if ((rc = download_blocks(h, nb, blocks, &flag)) != PGO_OK) return rc;
    if (!in_pattern)
        for (size_t k = 0; k < nb; ++k)
            if (!flag[k]) {
                c.err = "pgo_sparse_chol_selected_blocks: block " + std::to_string(k) + " (keyframes " + std::to_string(node_a[k]) + ", " + std::to_string(node_b[k]) + ") is not wholly in the pattern of the factor";
                return PGO_ERR_INVALID_ARG;
            }
    std::copy(blocks.begin(), blocks.end(), out);
    if (in_pattern) std::copy(flag.begin(), flag.end(), in_pattern);
    return PGO_OK;
}

int pgo_sparse_chol_inverse_columns(pgo_sparse_chol* h, int64_t n_cols, const int32_t* col_node, int64_t n_blocks, const int32_t* row_node, const int32_t* col_index, double* out) {
    if (!h) return PGO_ERR_INVALID_ARG;
    ScCore& c = h->c;
    c.err.clear();
    if (n_cols < 0 || n_cols > h->N || n_blocks < 0 || n_blocks > (int64_t)50000000 || (n_cols > 0 && !col_node) || (n_blocks > 0 && (!row_node || !col_index || !out))) {
        c.err = "pgo_sparse_chol_inverse_columns: null pointer or count out of range"; return PGO_ERR_INVALID_ARG;
    }
    if (!h->factored) { c.err = "pgo_sparse_chol_inverse_columns: no factor (pgo_sparse_chol_factor has not succeeded)"; return PGO_ERR_STATE; }
    const int nc = c.nc();
    const ScColumns Q(c.P, h->N, h->in_system.data(), h->pos.data(), n_cols, col_node, n_blocks, row_node, col_index, h->ws_limit);
    if (Q.error) { c.err = std::string("pgo_sparse_chol_inverse_columns: ") + Q.error; return PGO_ERR_INVALID_ARG; }
    const int64_t info[4] = {Q.launches, Q.products, Q.workspace, (int64_t)Q.chunks.size()};
    std::copy(info, info + 4, h->cols_info);
    if (n_blocks == 0) return PGO_OK;
    int rc;
    if ((rc = c.use()) != PGO_OK) return rc;
    const size_t nb = (size_t)n_blocks;
    std::vector<int32_t> tab;                              // every chunk's tables, one upload: rhs_col | first | row0
    std::vector<size_t> at;
    for (const ScColumnChunk& C : Q.chunks) {
        at.push_back(tab.size());
        tab.insert(tab.end(), C.rhs_col.begin(), C.rhs_col.end());
        tab.insert(tab.end(), C.first.begin(), C.first.end());
        tab.insert(tab.end(), C.row0.begin(), C.row0.end());
    }
    SCHIP(c.err, h->ws.ensure((size_t)Q.workspace));
    SCHIP(c.err, h->d_req.ensure(tab.size() * sizeof(int32_t)));
    SCHIP(c.err, h->d_na.ensure(nb * sizeof(int32_t))); SCHIP(c.err, h->d_nb.ensure(nb * sizeof(int32_t)));
    SCHIP(c.err, h->d_out.ensure(nb * 36 * sizeof(double)));
    SCHIP(c.err, hipMemcpyAsync(h->d_na.p, row_node, nb * sizeof(int32_t), hipMemcpyHostToDevice, c.st));
    SCHIP(c.err, hipMemcpyAsync(h->d_nb.p, col_index, nb * sizeof(int32_t), hipMemcpyHostToDevice, c.st));
    if (!tab.empty()) SCHIP(c.err, hipMemcpyAsync(h->d_req.p, tab.data(), tab.size() * sizeof(int32_t), hipMemcpyHostToDevice, c.st));
    SCHIP(c.err, hipEventRecord(c.e0, c.st));
    SCHIP(c.err, hipMemsetAsync(h->d_out.p, 0, nb * 36 * sizeof(double), c.st));
    double* W = h->ws.as<double>();
    for (size_t q = 0; q < Q.chunks.size(); ++q) {
        const ScColumnChunk& C = Q.chunks[q];
        const int32_t* d_col = h->d_req.as<const int32_t>() + at[q];
        const int32_t* d_first = d_col + C.rhs_col.size();
        const int32_t* d_row0 = d_first + C.first.size();
        SCHIP(c.err, hipMemsetAsync(W, 0, (size_t)C.m_pad * nc * sizeof(double), c.st));
        hipLaunchKernelGGL(sc_pcol_rhs_kernel, sc_grid(C.m_pad), dim3(SC_THREADS), 0, c.st, W, nc, C.m_pad, d_col);
        ScPanelLaunch L{c.T.as<const double>(), c.D, nc, W, d_first, c.st};
        sc_panel_steps(c.P, C.first, Q.k_stop, L);
        hipLaunchKernelGGL(sc_pgather_kernel, sc_grid((int64_t)nb * 36), dim3(SC_THREADS), 0, c.st, (const double*)W, nc, n_blocks, h->d_na.as<const int32_t>(),
                           h->d_nb.as<const int32_t>(), d_row0, h->d_in.as<const uint8_t>(), h->d_pos.as<const int32_t>(), h->d_out.as<double>());
    }
    std::vector<double> blocks;
    if ((rc = download_blocks(h, nb, blocks, nullptr)) != PGO_OK) return rc;
    std::copy(blocks.begin(), blocks.end(), out);
    return PGO_OK;
}

int pgo_sparse_chol_columns_info(const pgo_sparse_chol* h, int64_t* info4) {
    if (!h || !info4) return PGO_ERR_INVALID_ARG;
    std::copy(h->cols_info, h->cols_info + 4, info4);
    return PGO_OK;
}

int pgo_sparse_chol_set_workspace_limit(pgo_sparse_chol* h, int64_t bytes) {
    if (!h) return PGO_ERR_INVALID_ARG;
    h->c.err.clear();
    if (bytes < sc_panel_bytes(h->c.nc())) { h->c.err = "pgo_sparse_chol_set_workspace_limit: below one panel of right-hand sides, 64 rows of " + std::to_string(h->c.nc()) + " doubles"; return PGO_ERR_INVALID_ARG; }
    h->ws_limit = bytes;
    return PGO_OK;
}

int pgo_sparse_reduce_normal_blocks(int64_t n_nodes, const uint8_t* node_free, const double* diag, const double* offdiag, const double* sw_c, const double* sw_hss,
                                    int64_t n_rel, const int32_t* rel_c1, const int32_t* rel_c2, int64_t n_sw, const int32_t* swe_c1, const int32_t* swe_c2,
                                    int64_t* n_pairs, int32_t* pair_hi, int32_t* pair_lo, double* s_diag, double* s_blocks) {
    g_err.clear();
    const int64_t E = n_rel + n_sw;
    if (n_nodes < 1 || n_rel < 0 || n_sw < 0 || !node_free || !diag || !n_pairs || !s_diag || (E > 0 && (!offdiag || !pair_hi || !pair_lo || !s_blocks)) ||
        (n_rel > 0 && (!rel_c1 || !rel_c2)) || (n_sw > 0 && (!swe_c1 || !swe_c2 || !sw_c || !sw_hss))) {
        g_err = "pgo_sparse_reduce_normal_blocks: null pointer or negative count"; return PGO_ERR_INVALID_ARG;
    }
    const ScReduced R = sc_reduce_normal_blocks(n_nodes, node_free, diag, offdiag, sw_c, sw_hss, n_rel, rel_c1, rel_c2, n_sw, swe_c1, swe_c2);
    *n_pairs = (int64_t)R.pair_hi.size();
    std::copy(R.pair_hi.begin(), R.pair_hi.end(), pair_hi);
    std::copy(R.pair_lo.begin(), R.pair_lo.end(), pair_lo);
    std::copy(R.diag.begin(), R.diag.end(), s_diag);
    std::copy(R.blocks.begin(), R.blocks.end(), s_blocks);
    return PGO_OK;
}

}  // extern "C"

// the exact Levenberg-Marquardt step and solve on this factor (pgo_sparse_lm_*): kernels, object and entry points
#include "pgo_sparse_lm.hpp"

// a pose graph that linearises itself (pgo_sparse_graph_*): yaw/pitch/roll-weighted edges, and the exact LM solve without a pgo_problem handle
#include "pgo_sparse_graph.hpp"

// the reference's 4-DoF pose graph (pgo_sparse_yaw_graph_*): yaw + translation per keyframe, QinFourDOFWeightError edges, in the six-row slots of the exact LM step
#include "pgo_sparse_yaw.hpp"
