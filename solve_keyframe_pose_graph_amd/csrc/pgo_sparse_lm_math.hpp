// pgo_sparse_lm_math.hpp — the host side of the exact Levenberg-Marquardt step and solve of libpgo_sparse.so (include/pgo_sparse.h: pgo_sparse_lm_*): one LM system of
// a pose graph, damped and Schur-reduced from pgo_get_normal_blocks' arrays straight into the tile-sparse factor's tiles, solved exactly, the switches back-substituted
// and the model's cost change formed — Ceres' trust-region step with no tolerance, above PGO_DENSE_MAX_KEYFRAMES.  Here: the step plan (ScLmPlan), the per-entry
// arithmetic of one system as functions shared by the host and the kernels of pgo_sparse.hip (sc_lm_*), a serial host instantiation of the whole step on ScHost
// (ScLmHost; tests/native/sparse_lm_host.cpp) and the solve loop (sc_lm_solve), written once over a "stepper" — the device object or ScLmHost — around the decisions of
// pgo_lm.hpp, which is included unchanged: there is one controller.  libpgo.so does not include this header.
//
// The conventions are the handle's (pgo_kernels.hip: scale_init_kernel, lm_diag_kernel, sw_prepare_kernel, build_rows_kernel, model_change_kernel; pgo_solver.hip):
//   scale      S_j = 1 / (1 + sqrt(H_jj)) per column, H_jj from `diag` (pose columns, BEFORE the switch elimination) and `sw_hss`; fixed at iteration 0
//   damping    lambda_j = clamp(S_j^2 H_jj, min_lm_diagonal, max_lm_diagonal) / (radius S_j^2): the clamp applies in scaled coordinates, lambda is added in unscaled ones
//   pivot      a_e = 1 / (h_e + lambda_e)
//   system     (H_pp + diag(lambda_p) - sum_e c_e a_e c_e^T) dp = -(g_p - sum_e c_e a_e g_s,e), block by block, the Schur terms taken off first, lambda added last
//   switches   ds_e = -a_e (g_s,e + c_e^T dp)
//   model      model_cost_change = -d^T (g + H d / 2) with the full undamped H: pose diagonal blocks, J1^T J2 per edge both ways, switch couplings, h_e
// A robust edge enters through its corrected blocks (pgo_get_normal_blocks returns them): nothing here knows of losses.  The step norm and x_norm of the controller are
// ambient (|x - Plus(x, d)| over 4 + 3 numbers per keyframe and one per switch): the solve loop forms them from the candidate; a single step reports the tangent norm |d|.
#pragma once
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "pgo_lm.hpp"
#include "pgo_sparse_blocks.hpp"

namespace pgo {

// ---- the step plan, built once per graph.  All lists are CSR over int32: what a kernel needs to write each block once, as a sum in a fixed order.
//   side:  per keyframe of the system the switchable edge sides incident to it, edge << 1 | side, in edge order;
//   pair:  per pair k of the factor's pair list (rows of pair_hi[k], columns of pair_lo[k], as pgo_sparse_chol_create took them) the edges on it in internal edge order
//          (relative-pose in add order, then switchable: the order of pgo_get_normal_blocks' offdiag): index inside its class << 2 | switchable << 1 | transposed
//          (the edge's c1 is pair_lo[k]: J1^T J2 is read transposed);
//   inc:   per keyframe of the system every edge side incident to it, internal edge index << 1 | side, in edge order: the rows of H d are pulled over it.
// A keyframe outside the system — constant, or referenced by no residual block (in_system = 0 in pgo_sparse_chol_create) — has empty lists and its rows and columns
// drop out; an edge side that touches one drops out of the pair list (the edge is on no pair), and a switch whose both endpoints are outside keeps its pivot alone.
struct ScLmPlan {
    int64_t N = 0, n_rel = 0, n_sw = 0, n_pairs = 0;
    std::vector<uint8_t> in_sys;
    std::vector<int32_t> side_ptr, side, pair_ptr, pair_ent, inc_ptr, inc, c1, c2;      // c1, c2: [n_rel + n_sw], internal edge order
    const char* error = nullptr;
    ScLmPlan() = default;
    ScLmPlan(int64_t n_nodes, const uint8_t* in_system, const uint8_t* node_free, int64_t np, const int32_t* pair_hi, const int32_t* pair_lo, int64_t nr, const int32_t* rc1, const int32_t* rc2,
             int64_t ns, const int32_t* sc1, const int32_t* sc2) : N(n_nodes), n_rel(nr), n_sw(ns), n_pairs(np) {
        if (nr + ns >= ((int64_t)1 << 29)) { error = "more than 2^29 edges"; return; }
        in_sys.assign((size_t)N, 0);
        for (int64_t i = 0; i < N; ++i) in_sys[(size_t)i] = in_system[i] && node_free[i] ? 1 : 0;
        const int64_t E = nr + ns;
        c1.resize((size_t)E); c2.resize((size_t)E);
        for (int64_t e = 0; e < E; ++e) {
            const int32_t a = e < nr ? rc1[e] : sc1[e - nr], b = e < nr ? rc2[e] : sc2[e - nr];
            if (a < 0 || b < 0 || a >= N || b >= N) { error = "an edge names a keyframe out of range"; return; }
            if (a == b) { error = "an edge joins a keyframe with itself"; return; }
            for (int32_t nd : {a, b}) if (node_free[nd] && !in_system[nd]) { error = "an edge touches a free keyframe that the factor keeps outside the system"; return; }
            c1[(size_t)e] = a; c2[(size_t)e] = b;
        }
        // the factor's pairs, found by (higher, lower)
        std::vector<std::pair<std::pair<int32_t, int32_t>, int32_t>> key((size_t)np);
        for (int64_t k = 0; k < np; ++k) key[(size_t)k] = {{std::max(pair_hi[k], pair_lo[k]), std::min(pair_hi[k], pair_lo[k])}, (int32_t)k};
        std::sort(key.begin(), key.end());
        auto pair_of = [&](int32_t a, int32_t b) -> int32_t {
            const std::pair<int32_t, int32_t> want{std::max(a, b), std::min(a, b)};
            auto it = std::lower_bound(key.begin(), key.end(), std::make_pair(want, (int32_t)-1));
            return it != key.end() && it->first == want ? it->second : -1;
        };
        side_ptr.assign((size_t)N + 1, 0); inc_ptr.assign((size_t)N + 1, 0); pair_ptr.assign((size_t)np + 1, 0);
        std::vector<int32_t> on((size_t)E, -1);
        for (int64_t e = 0; e < E; ++e) {
            const int32_t a = c1[(size_t)e], b = c2[(size_t)e];
            for (int32_t nd : {a, b}) if (in_sys[(size_t)nd]) { ++inc_ptr[(size_t)nd + 1]; if (e >= nr) ++side_ptr[(size_t)nd + 1]; }
            if (!in_sys[(size_t)a] || !in_sys[(size_t)b]) continue;
            if ((on[(size_t)e] = pair_of(a, b)) < 0) { error = "an edge joins two keyframes of the system that are no pair of the factor"; return; }
            ++pair_ptr[(size_t)on[(size_t)e] + 1];
        }
        for (int64_t i = 0; i < N; ++i) { side_ptr[(size_t)i + 1] += side_ptr[(size_t)i]; inc_ptr[(size_t)i + 1] += inc_ptr[(size_t)i]; }
        for (int64_t k = 0; k < np; ++k) pair_ptr[(size_t)k + 1] += pair_ptr[(size_t)k];
        side.assign((size_t)side_ptr[(size_t)N], 0); inc.assign((size_t)inc_ptr[(size_t)N], 0); pair_ent.assign((size_t)pair_ptr[(size_t)np], 0);
        std::vector<int32_t> fs(side_ptr.begin(), side_ptr.end() - 1), fi(inc_ptr.begin(), inc_ptr.end() - 1), fp(pair_ptr.begin(), pair_ptr.end() - 1);
        for (int64_t e = 0; e < E; ++e)      // (edges ascending: every list comes out in internal edge order)
            for (int s = 0; s < 2; ++s) {
                const int32_t nd = s ? c2[(size_t)e] : c1[(size_t)e];
                if (!in_sys[(size_t)nd]) continue;
                inc[(size_t)fi[(size_t)nd]++] = (int32_t)((e << 1) | s);
                if (e >= nr) side[(size_t)fs[(size_t)nd]++] = (int32_t)(((e - nr) << 1) | s);
            }
        for (int64_t e = 0; e < E; ++e) {
            const int32_t k = on[(size_t)e];
            if (k < 0) continue;
            const bool sw = e >= nr, tr = c1[(size_t)e] == pair_lo[k];
            pair_ent[(size_t)fp[(size_t)k]++] = (int32_t)(((sw ? e - nr : e) << 2) | (sw ? 2 : 0) | (tr ? 1 : 0));
        }
    }
};

// ---- everything one step reads and writes, as plain pointers: the same struct on the host and, by value, as a kernel argument
struct ScLmView {
    int64_t N, n_rel, n_sw, n_pairs;
    int nc;                                                   // order of the padded matrix
    const uint8_t* in_sys; const int32_t* pos;                // [N]
    const int32_t *side_ptr, *side, *pair_ptr, *pair_ent, *pair_hi, *pair_lo, *inc_ptr, *inc, *c1, *c2;
    const double *diag, *grad, *offdiag, *sw_c, *sw_hss, *sw_gs;      // pgo_get_normal_blocks' arrays
    const double *scale_p, *scale_s;                          // [6 N], [n_sw]: S, fixed at iteration 0
    double *lam, *a_inv;                                      // [6 N], [n_sw]: the damping of the pose columns, the damped switch pivots
};

// ---- the per-entry arithmetic
PGO_DC_HD double sc_lm_scale(double h) { return 1.0 / (1.0 + sqrt(h)); }
PGO_DC_HD double sc_lm_lambda(double s, double h, double mn, double mx, double radius) { return fmin(fmax(s * s * h, mn), mx) / (radius * s * s); }
PGO_DC_HD double sc_lm_pivot(double h, double lam) { return 1.0 / (h + lam); }

// column j < 6 N + n_sw of the damping: lam (0 for a keyframe outside the system) or the switch's damped pivot.  Returns true when that pivot is not > 0 (or NaN).
PGO_DC_HD bool sc_lm_damp_column(const ScLmView& V, int64_t j, double radius, double mn, double mx) {
    if (j < V.N * 6) {
        const int64_t n = j / 6; const int c = (int)(j - n * 6);
        V.lam[j] = V.in_sys[n] ? sc_lm_lambda(V.scale_p[j], V.diag[n * 36 + c * 7], mn, mx, radius) : 0.0;
        return false;
    }
    const int64_t e = j - V.N * 6;
    const double d = V.sw_hss[e] + sc_lm_lambda(V.scale_s[e], V.sw_hss[e], mn, mx, radius);
    V.a_inv[e] = 1.0 / d;
    return dc_bad_pivot(d) || dc_bad_hss(d);
}
// entry (a, c) of keyframe i's diagonal block of the damped Schur complement
PGO_DC_HD double sc_lm_diag_entry(const ScLmView& V, int64_t i, int a, int c) {
    double acc = V.diag[i * 36 + a * 6 + c];
    for (int32_t k = V.side_ptr[i]; k < V.side_ptr[i + 1]; ++k) {
        const int32_t w = V.side[k];
        const double* cc = V.sw_c + (size_t)(w >> 1) * 12 + (w & 1) * 6;
        const double sq = cc[a] * cc[c];
        acc = acc - sq * V.a_inv[w >> 1];
    }
    return a == c ? acc + V.lam[i * 6 + a] : acc;
}
// entry (a, c) of the block of pair k: rows of pair_hi[k], columns of pair_lo[k]
PGO_DC_HD double sc_lm_pair_entry(const ScLmView& V, int64_t k, int a, int c) {
    double acc = 0.0;
    for (int32_t q = V.pair_ptr[k]; q < V.pair_ptr[k + 1]; ++q) {
        const int32_t w = V.pair_ent[q];
        const bool tr = (w & 1) != 0, sw = (w & 2) != 0;
        const size_t idx = (size_t)(w >> 2);
        const double* H = V.offdiag + ((sw ? (size_t)V.n_rel : 0) + idx) * 36;
        double v = tr ? H[c * 6 + a] : H[a * 6 + c];
        if (sw) {
            const double* cc = V.sw_c + idx * 12;
            const double cross = cc[(tr ? 6 : 0) + a] * cc[(tr ? 0 : 6) + c];
            v = v - cross * V.a_inv[idx];
        }
        acc = acc + v;
    }
    return acc;
}
// entry a of keyframe i's reduced right-hand side
PGO_DC_HD double sc_lm_rhs_entry(const ScLmView& V, int64_t i, int a) {
    double acc = -V.grad[i * 6 + a];
    for (int32_t k = V.side_ptr[i]; k < V.side_ptr[i + 1]; ++k) {
        const int32_t w = V.side[k];
        const size_t e = (size_t)(w >> 1);
        const double gsa = V.sw_gs[e] * V.a_inv[e];
        acc = acc + V.sw_c[e * 12 + (w & 1) * 6 + a] * gsa;
    }
    return acc;
}
// What thread gid of the fill writes — 36 entries per keyframe, the padding, 36 per pair (sc_fill_kernel's layout): its place in the permuted matrix's lower triangle
// and its value.  false: nothing (above the diagonal of a diagonal block, an off-diagonal entry of a keyframe outside the system, past the end).
PGO_DC_HD bool sc_lm_fill_entry(const ScLmView& V, int64_t gid, int* row, int* col, double* v) {
    const int64_t n36 = V.N * 36, pad = (int64_t)V.nc - V.N * 6;
    if (gid < n36) {
        const int64_t node = gid / 36;
        const int e = (int)(gid - node * 36), a = e / 6, c = e - a * 6;
        if (!sc_block_entry(V.pos[node], V.pos[node], a, c, row, col)) return false;
        if (V.in_sys[node]) *v = sc_lm_diag_entry(V, node, a, c);
        else if (a == c) *v = 1.0;
        else return false;
        return true;
    }
    if (gid < n36 + pad) { *row = *col = (int)(V.N * 6 + (gid - n36)); *v = 1.0; return true; }
    const int64_t u = gid - n36 - pad, k = u / 36;
    if (k >= V.n_pairs) return false;
    const int e = (int)(u - k * 36), a = e / 6, c = e - a * 6;
    sc_block_entry(V.pos[V.pair_hi[k]], V.pos[V.pair_lo[k]], a, c, row, col);
    *v = sc_lm_pair_entry(V, k, a, c);
    return true;
}
PGO_DC_HD int64_t sc_lm_fill_threads(const ScLmView& V) { return V.N * 36 + ((int64_t)V.nc - V.N * 6) + V.n_pairs * 36; }

// the step of switch e from the solution x of the reduced system in the factor's order (x: nc doubles, keyframe i at 6 pos[i])
PGO_DC_HD double sc_lm_backsub(const ScLmView& V, int64_t e, const double* x) {
    const int32_t n1 = V.c1[V.n_rel + e], n2 = V.c2[V.n_rel + e];
    const double* cc = V.sw_c + e * 12;
    double acc = V.sw_gs[e];
    if (V.in_sys[n1]) { const double* d = x + (size_t)V.pos[n1] * 6; for (int i = 0; i < 6; ++i) acc = acc + cc[i] * d[i]; }
    if (V.in_sys[n2]) { const double* d = x + (size_t)V.pos[n2] * 6; for (int i = 0; i < 6; ++i) acc = acc + cc[6 + i] * d[i]; }
    return -acc * V.a_inv[e];
}
// Item `it` < N + n_sw of the model: a keyframe's or a switch's share of d^T g, d^T H d and d^T d with the full undamped H.  dp [6 N] in the caller's keyframe order
// (zero outside the system), ds [n_sw].  A keyframe's rows of H d are pulled over its incident edge sides in list order.
PGO_DC_HD void sc_lm_model_item(const ScLmView& V, int64_t it, const double* dp, const double* ds, double* dg, double* dhd, double* dd) {
    *dg = *dhd = *dd = 0.0;
    if (it < V.N) {
        if (!V.in_sys[it]) return;
        double d[6], y[6];
        for (int a = 0; a < 6; ++a) d[a] = dp[it * 6 + a];
        const double* H = V.diag + it * 36;
        for (int a = 0; a < 6; ++a) { double s = 0.0; for (int c = 0; c < 6; ++c) s = s + H[a * 6 + c] * d[c]; y[a] = s; }
        for (int32_t k = V.inc_ptr[it]; k < V.inc_ptr[it + 1]; ++k) {
            const int32_t w = V.inc[k];
            const int64_t E = w >> 1;
            const int side = w & 1;
            const double* o = dp + (size_t)(side ? V.c1[E] : V.c2[E]) * 6;
            const double* B = V.offdiag + E * 36;
            for (int a = 0; a < 6; ++a) { double s = 0.0; for (int c = 0; c < 6; ++c) s = s + (side ? B[c * 6 + a] : B[a * 6 + c]) * o[c]; y[a] = y[a] + s; }
            if (E >= V.n_rel) { const int64_t es = E - V.n_rel; const double dse = ds[es]; for (int a = 0; a < 6; ++a) y[a] = y[a] + V.sw_c[es * 12 + side * 6 + a] * dse; }
        }
        double g = 0.0, h = 0.0, n2 = 0.0;
        for (int a = 0; a < 6; ++a) { g = g + d[a] * V.grad[it * 6 + a]; h = h + d[a] * y[a]; n2 = n2 + d[a] * d[a]; }
        *dg = g; *dhd = h; *dd = n2;
        return;
    }
    const int64_t e = it - V.N;
    const double dse = ds[e];
    const double* cc = V.sw_c + e * 12;
    const double* d1 = dp + (size_t)V.c1[V.n_rel + e] * 6; const double* d2 = dp + (size_t)V.c2[V.n_rel + e] * 6;
    double y = V.sw_hss[e] * dse;
    for (int i = 0; i < 6; ++i) y = y + cc[i] * d1[i] + cc[6 + i] * d2[i];
    *dg = dse * V.sw_gs[e]; *dhd = dse * y; *dd = dse * dse;
}
// the model's items are summed by chunks of SC_LM_CHUNK (one workgroup each on the device: a fixed binary tree), the chunks' partial sums in ascending order
constexpr int SC_LM_CHUNK = 256;
PGO_DC_HD double sc_lm_model_cost_change(double dg, double dhd) { return -(dg + 0.5 * dhd); }

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- serial host instantiation of one step on ScHost: the reference of the kernels.  The owner keeps the plan, the factor's plan and pos alive.
struct ScLmHost {
    const ScLmPlan& L; const ScPlan& P; const int32_t* pos; const int32_t* pair_hi; const int32_t* pair_lo;
    std::vector<double> scale_p, scale_s, lam, a_inv, T, w, yv, x;
    bool scale_set = false;
    double factor_ms = 0.0;
    ScLmHost(const ScLmPlan& l, const ScPlan& p, const int32_t* ps, const int32_t* hi, const int32_t* lo) : L(l), P(p), pos(ps), pair_hi(hi), pair_lo(lo) {
        scale_p.assign((size_t)L.N * 6, 1.0); scale_s.assign((size_t)L.n_sw, 1.0); lam.assign((size_t)L.N * 6, 0.0); a_inv.assign((size_t)L.n_sw, 0.0);
    }
    ScLmView view(const double* diag, const double* grad, const double* offdiag, const double* sw_c, const double* sw_hss, const double* sw_gs) {
        return ScLmView{L.N, L.n_rel, L.n_sw, L.n_pairs, P.nt * DC_NB, L.in_sys.data(), pos, L.side_ptr.data(), L.side.data(), L.pair_ptr.data(), L.pair_ent.data(), pair_hi, pair_lo,
                        L.inc_ptr.data(), L.inc.data(), L.c1.data(), L.c2.data(), diag, grad, offdiag, sw_c, sw_hss, sw_gs, scale_p.data(), scale_s.data(), lam.data(), a_inv.data()};
    }
    // diag = nullptr: no Jacobi scaling, S = 1
    int set_scale(const double* diag, const double* sw_hss) {
        for (int64_t j = 0; j < L.N * 6; ++j) scale_p[(size_t)j] = diag ? sc_lm_scale(diag[(j / 6) * 36 + (j % 6) * 7]) : 1.0;
        for (int64_t e = 0; e < L.n_sw; ++e) scale_s[(size_t)e] = diag ? sc_lm_scale(sw_hss[e]) : 1.0;
        scale_set = true;
        return PGO_OK;
    }
    // the damped Schur complement in the tiles T and the reduced right-hand side in w; false: a switch pivot is not > 0
    bool assemble(const ScLmView& V, double radius, double mn, double mx) {
        bool bad = false;
        for (int64_t j = 0; j < L.N * 6 + L.n_sw; ++j) bad = sc_lm_damp_column(V, j, radius, mn, mx) || bad;
        T.assign((size_t)P.tiles() * SC_TILE, 0.0);
        int row, col; double v;
        for (int64_t gid = 0; gid < sc_lm_fill_threads(V); ++gid)
            if (sc_lm_fill_entry(V, gid, &row, &col, &v)) T[(size_t)P.find(row / DC_NB, col / DC_NB) * SC_TILE + (size_t)(row % DC_NB) * DC_NB + col % DC_NB] = v;
        w.assign((size_t)V.nc, 0.0);
        for (int64_t i = 0; i < L.N; ++i) if (L.in_sys[(size_t)i]) for (int a = 0; a < 6; ++a) w[(size_t)pos[i] * 6 + a] = sc_lm_rhs_entry(V, i, a);
        return !bad;
    }
    // PGO_OK, PGO_ERR_STATE (no scale) or PGO_ERR_NUMERIC (a pivot is not > 0: nothing is written).  out3: model cost change, |d|, the factor's milliseconds.
    int step(const double* diag, const double* grad, const double* offdiag, const double* sw_c, const double* sw_hss, const double* sw_gs, double radius, double mn, double mx, double* delta_pose,
             double* delta_sw, double* out3) {
        if (!scale_set) return PGO_ERR_STATE;
        const ScLmView V = view(diag, grad, offdiag, sw_c, sw_hss, sw_gs);
        const bool ok = assemble(V, radius, mn, mx);
        yv.assign((size_t)V.nc, 0.0); x.assign((size_t)V.nc, 0.0);
        ScHost H{P, T.data(), w.data(), yv.data(), x.data()};
        const auto t0 = std::chrono::steady_clock::now();
        sc_factor_steps(P, H);
        factor_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (!ok || H.failed) return PGO_ERR_NUMERIC;
        sc_solve_steps(P, H);
        std::vector<double> dp((size_t)L.N * 6, 0.0), ds((size_t)L.n_sw, 0.0);
        for (int64_t i = 0; i < L.N; ++i) if (L.in_sys[(size_t)i]) for (int a = 0; a < 6; ++a) dp[(size_t)i * 6 + a] = x[(size_t)pos[i] * 6 + a];
        for (int64_t e = 0; e < L.n_sw; ++e) ds[(size_t)e] = sc_lm_backsub(V, e, x.data());
        double dg = 0.0, dhd = 0.0, dd = 0.0;
        for (int64_t c0 = 0; c0 < L.N + L.n_sw; c0 += SC_LM_CHUNK) {
            double a = 0.0, b = 0.0, c = 0.0, g, h, n2;
            for (int64_t it = c0; it < std::min<int64_t>(c0 + SC_LM_CHUNK, L.N + L.n_sw); ++it) { sc_lm_model_item(V, it, dp.data(), ds.data(), &g, &h, &n2); a += g; b += h; c += n2; }
            dg += a; dhd += b; dd += c;
        }
        std::copy(dp.begin(), dp.end(), delta_pose);
        if (L.n_sw) std::copy(ds.begin(), ds.end(), delta_sw);
        out3[0] = sc_lm_model_cost_change(dg, dhd); out3[1] = std::sqrt(dd); out3[2] = factor_ms;
        return PGO_OK;
    }
};
#endif

// ---- the solve loop, once for every stepper (set_scale / step as ScLmHost has them).  The callbacks have the signatures of pgo_evaluate, pgo_get_normal_blocks and
// pgo_manifold_plus without the handle; a non-zero return ends the solve with that code and leaves the arrays alone.
struct ScLmCallbacks {
    int (*evaluate)(void* user, const double* quat, const double* t, const double* sw, int64_t n_nodes, int64_t n_switch, double* cost, double* residuals, double* gradient);
    int (*normal_blocks)(void* user, double* diag, double* grad, double* offdiag, double* sw_c, double* sw_hss, double* sw_gs);
    int (*manifold_plus)(void* user, int64_t n, const double* quat, const double* t, const double* delta, double* quat_out, double* t_out);
};
inline double sc_lm_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// swe_index [n_sw]: the switch index of every switchable edge (nullptr: edge e uses switch e).  lm_begin, lm_pre_step, lm_step_outcome, lm_outcome_stop, lm_finish_step
// around the stepper: a candidate is Plus(x, dp) through the callback and sw + ds, evaluated for its cost alone; an accepted step is linearised again; a failed
// factorisation (PGO_ERR_NUMERIC of the stepper) is an invalid step, PGO_STEP_INVALID_FACTORIZATION, and the radius halves.  No pause plan: every step is exact.
template <class Stepper>
inline int sc_lm_solve(Stepper& S, const ScLmPlan& L, const ScLmCallbacks& cb, void* user, int64_t n_switch, const int32_t* swe_index, double* quat, double* t, double* sw, const pgo_options& o,
                       pgo_summary* out) {
    const int64_t N = L.N, E = L.n_rel + L.n_sw, Es = L.n_sw;
    const double t_begin = sc_lm_now();
    pgo_summary sum;
    std::memset(&sum, 0, sizeof(sum));
    sum.termination_type = PGO_NO_CONVERGENCE;
    std::vector<double> q(quat, quat + N * 4), tt(t, t + N * 3), s(sw ? sw : nullptr, sw ? sw + n_switch : nullptr), qn((size_t)N * 4), tn((size_t)N * 3), sn(s);
    std::vector<double> diag((size_t)N * 36), grad((size_t)N * 6), off((size_t)E * 36), c((size_t)Es * 12), hss((size_t)Es), gs((size_t)Es), full((size_t)N * 6 + (size_t)n_switch), neg((size_t)N * 6);
    std::vector<double> dp((size_t)N * 6), ds((size_t)Es);
    auto swi = [&](int64_t e) { return swe_index ? (int64_t)swe_index[e] : e; };
    for (int64_t e = 0; e < Es; ++e) if (swi(e) < 0 || swi(e) >= n_switch) return PGO_ERR_INVALID_ARG;
    LmState lm = lm_begin(o);
    int rc;
    // K1 + K2 at (q, tt, s): cost, normal blocks, x_norm and the projected-gradient max norm |Plus(x, -g) - x|_inf, as linearize() of the handle forms them
    auto linearize = [&](double* cost) -> int {
        if ((rc = cb.evaluate(user, q.data(), tt.data(), n_switch ? s.data() : nullptr, N, n_switch, cost, nullptr, full.data())) != PGO_OK) return rc;
        if ((rc = cb.normal_blocks(user, diag.data(), grad.data(), E ? off.data() : nullptr, Es ? c.data() : nullptr, Es ? hss.data() : nullptr, Es ? gs.data() : nullptr)) != PGO_OK) return rc;
        for (int64_t i = 0; i < N; ++i) for (int a = 0; a < 6; ++a) neg[(size_t)i * 6 + a] = a < 3 ? -grad[(size_t)i * 6 + a] : 0.0;
        if ((rc = cb.manifold_plus(user, N, q.data(), nullptr, neg.data(), qn.data(), nullptr)) != PGO_OK) return rc;
        double x2 = 0.0, gm = 0.0;
        for (int64_t i = 0; i < N; ++i) {
            if (!L.in_sys[(size_t)i]) continue;
            for (int k = 0; k < 4; ++k) { x2 += q[(size_t)i * 4 + k] * q[(size_t)i * 4 + k]; gm = std::fmax(gm, std::fabs(qn[(size_t)i * 4 + k] - q[(size_t)i * 4 + k])); }
            for (int k = 0; k < 3; ++k) { x2 += tt[(size_t)i * 3 + k] * tt[(size_t)i * 3 + k]; gm = std::fmax(gm, std::fabs(grad[(size_t)i * 6 + 3 + k])); }
        }
        for (int64_t e = 0; e < Es; ++e) { x2 += s[(size_t)swi(e)] * s[(size_t)swi(e)]; gm = std::fmax(gm, std::fabs(gs[(size_t)e])); }
        lm.x_norm = std::sqrt(x2); lm.gmax = gm;
        return PGO_OK;
    };
    auto log_iter = [&](const pgo_iteration& it) { if (sum.num_logged < PGO_MAX_ITERATION_LOG) sum.iterations[sum.num_logged++] = it; };
    auto terminate = [&](int type, const char* msg) { lm.terminated = true; sum.termination_type = type; std::snprintf(sum.message, sizeof(sum.message), "%s", msg); };
    if ((rc = linearize(&lm.x_cost)) != PGO_OK) return rc;
    if ((rc = S.set_scale(o.jacobi_scaling ? diag.data() : nullptr, hss.data())) != PGO_OK) return rc;
    sum.initial_cost = sum.final_cost = lm.x_cost;
    if (!std::isfinite(lm.x_cost)) terminate(PGO_FAILURE, "initial cost is not finite");
    else {
        pgo_iteration it{};
        it.step_is_valid = 1; it.step_is_successful = 1; it.cost = lm.x_cost; it.gradient_max_norm = lm.gmax; it.trust_region_radius = lm.radius; it.seconds = sc_lm_now() - t_begin;
        log_iter(it);
    }
    while (!lm.terminated) {
        const LmStop before = lm_pre_step(lm, o, false);
        if (before.message) { terminate(before.type, before.message); break; }
        const double t0 = sc_lm_now();
        ++lm.iteration;
        pgo_iteration it{};
        it.iteration = lm.iteration; it.trust_region_radius = lm.radius; it.preconditioner = PGO_PRECOND_DIRECT;
        double out3[3] = {0.0, 0.0, 0.0};
        rc = S.step(diag.data(), grad.data(), off.data(), c.data(), hss.data(), gs.data(), lm.radius, o.min_lm_diagonal, o.max_lm_diagonal, dp.data(), ds.data(), out3);
        if (rc != PGO_OK && rc != PGO_ERR_NUMERIC) return rc;
        const int why_invalid = rc == PGO_OK ? PGO_STEP_ACCEPTED : PGO_STEP_INVALID_FACTORIZATION;
        const double t_solved = sc_lm_now();
        it.seconds_system = out3[2] * 1e-3; it.seconds_pcg = (t_solved - t0) - it.seconds_system;
        LmCandidate cand{};
        if (rc == PGO_OK) {
            if ((rc = cb.manifold_plus(user, N, q.data(), tt.data(), dp.data(), qn.data(), tn.data())) != PGO_OK) return rc;
            double s2 = 0.0;
            for (int64_t i = 0; i < N; ++i) {
                if (!L.in_sys[(size_t)i]) { std::copy(q.begin() + i * 4, q.begin() + i * 4 + 4, qn.begin() + i * 4); std::copy(tt.begin() + i * 3, tt.begin() + i * 3 + 3, tn.begin() + i * 3); continue; }
                for (int k = 0; k < 4; ++k) { const double d = q[(size_t)i * 4 + k] - qn[(size_t)i * 4 + k]; s2 += d * d; }
                for (int k = 0; k < 3; ++k) { const double d = tt[(size_t)i * 3 + k] - tn[(size_t)i * 3 + k]; s2 += d * d; }
            }
            sn = s;
            for (int64_t e = 0; e < Es; ++e) { sn[(size_t)swi(e)] = s[(size_t)swi(e)] + ds[(size_t)e]; s2 += ds[(size_t)e] * ds[(size_t)e]; }
            double cost = 0.0;
            if ((rc = cb.evaluate(user, qn.data(), tn.data(), n_switch ? sn.data() : nullptr, N, n_switch, &cost, nullptr, nullptr)) != PGO_OK) return rc;
            cand = LmCandidate{cost, out3[0], std::sqrt(s2)};
            it.seconds_evaluate = sc_lm_now() - t_solved;
        }
        const LmOutcome outc = lm_step_outcome(lm, o, false, why_invalid, false, cand, &it);
        double new_cost = lm.x_cost;
        if (outc == LmOutcome::accepted) {
            q.swap(qn); tt.swap(tn); s.swap(sn);
            const double t_lin = sc_lm_now();
            if ((rc = linearize(&new_cost)) != PGO_OK) return rc;
            it.seconds_linearize = sc_lm_now() - t_lin;
        } else if (outc == LmOutcome::invalid) {
            // the blocks of the present point are fetched again: a handle gives the numbers it gave before, and the next step does not depend on arrays a failed step has seen
            double same = 0.0;
            if ((rc = linearize(&same)) != PGO_OK) return rc;
        }
        lm_finish_step(lm, o, outc, it.relative_decrease, new_cost);
        if (outc == LmOutcome::accepted) ++sum.num_successful_steps; else if (!it.step_is_valid || outc == LmOutcome::rejected) ++sum.num_unsuccessful_steps;
        const LmStop after = lm_outcome_stop(outc);
        if (after.message) terminate(after.type, after.message);
        it.cost = lm.x_cost; it.gradient_max_norm = lm.gmax; it.seconds = sc_lm_now() - t0;
        log_iter(it);
        sum.final_cost = lm.x_cost;
    }
    sum.num_iterations = lm.iteration;
    sum.final_cost = lm.x_cost;
    sum.seconds_device = sum.seconds_total = sc_lm_now() - t_begin;
    if (sum.termination_type != PGO_FAILURE) {      // (on PGO_FAILURE the arrays are left unmodified)
        std::copy(q.begin(), q.end(), quat); std::copy(tt.begin(), tt.end(), t);
        if (sw) std::copy(s.begin(), s.end(), sw);
    }
    if (out) *out = sum;
    return PGO_OK;
}

}  // namespace pgo
