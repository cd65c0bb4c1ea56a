// pgo_sparse_yaw_math.hpp — the linearisation of pgo_sparse_yaw_graph (include/pgo_sparse.h) per item, host and device (PGO_HD): what the kernels of pgo_sparse_yaw.hpp run
// one thread per item and what a serial host instantiation (tests/native/sparse_yaw_host.cpp) runs in a loop.  Plain C++: no HIP call.
//
// The graph is the reference's 4-DoF formulation (__USE_YPR_REP, VINS-Fusion's): a keyframe is a yaw angle in DEGREES and a translation, every edge a
// QinFourDOFWeightError (src/CeresResidues.h:426-546) with the pitch and roll of its first keyframe as constants, the yaw on AngleLocalParameterization.
//
//   sy_normalize        the reference's NormalizeAngle: ONE conditional fold by 360, not an fmod;
//   sy_residual         the functor in closed form with its analytic Jacobians, 4 x 4 per side in the tangent [psi, t];
//   sy_block_item       one edge: the residual, 0.5 |r|^2, and with Jacobians J1, J2 into the block store and J1^T J2 into its 6 x 6 place of offdiag;
//   sy_node_item        a keyframe's diag and grad over its incident list in list order, the two unit pad entries;
//   sy_plus_item        psi+ = N(psi + dpsi), t+ = t + dt.
// SyGraph is the host model: the edges as they were added, their validation (every PGO_ERR_INVALID_ARG of the interface) and the tables of _finalize; SyHostLin the serial
// instantiation.  Every address the items touch comes from these tables, none from the numbers.
//
// The embedding in the six-row slots of pgo_sparse_lm_step and sc_lm_solve: ambient quat[4 i] = psi_i, quat[4 i + 1 .. 3] = 0, t[3 i ..]; tangent delta[6 i] = dpsi,
// delta[6 i + 1] = delta[6 i + 2] = 0 (pad), delta[6 i + 3 .. 5] = dt.  Column k of a 4-wide Jacobian sits at 6-wide column SY_SLOT(k) = 0, 3, 4, 5.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "pgo.h"
#include "pgo_device_math.hpp"

namespace pgo {

constexpr int SY_EDGE_DOUBLES = 7;      // t_meas[3] rel_yaw pitch_i roll_i w
constexpr int SY_CHUNK = 256;           // cost terms per partial sum: a workgroup of the block kernel
constexpr double SY_PI = 3.14159265358979323846;

// NormalizeAngle as it is: 180 stays 180, 400 becomes 40, 800 becomes 440
PGO_HD double sy_normalize(double a) {
    if (a > 180.0) return a - 360.0;
    if (a < -180.0) return a + 360.0;
    return a;
}

// ---------------------------------------------------------------------------------------------
// QinFourDOFWeightError of edge (i, j) with the record rec = (t_meas[3], rel_yaw, pitch_i, roll_i, w), angles in degrees:
//   R_i = Rz(psi_i) Ry(pitch_i) Rx(roll_i)   (YawPitchRollToRotationMatrix)
//   r[0..2] = w (R_i^T (t_j - t_i) - t_meas)        r[3] = w N(psi_j - psi_i - rel_yaw) / 10
// J1 [16], J2 [16]: 4 x 4 row-major, columns [psi, t(3)] of keyframe i / j.  With d = t_j - t_i and dR/dpsi = Rz' Ry Rx (row 0 of it is -row 1 of R, row 1 is row 0, row 2 zero):
//   dr[a]/dt_j[b] = w R[b][a]      dr[a]/dt_i[b] = -w R[b][a]      dr[a]/dpsi_i = w (pi / 180) (R[0][a] d[1] - R[1][a] d[0])      dr[3]/dpsi_j = w / 10 = -dr[3]/dpsi_i
// (N has slope 1 wherever it is differentiable; the parameterisation's Jacobian is 1).
// ---------------------------------------------------------------------------------------------
template <bool WANT_J>
PGO_HD void sy_residual(double psi_i, double ti0, double ti1, double ti2, double psi_j, double tj0, double tj1, double tj2, const double* rec, double* r4, double* J1, double* J2) {
    const double y = psi_i / 180.0 * SY_PI, p = rec[4] / 180.0 * SY_PI, ro = rec[5] / 180.0 * SY_PI, w = rec[6];
    const double cy = cos(y), sy = sin(y), cp = cos(p), sp = sin(p), cr = cos(ro), sr = sin(ro);
    const double R00 = cy * cp, R01 = -sy * cr + cy * sp * sr, R02 = sy * sr + cy * sp * cr;
    const double R10 = sy * cp, R11 = cy * cr + sy * sp * sr, R12 = -cy * sr + sy * sp * cr;
    const double R20 = -sp, R21 = cp * sr, R22 = cp * cr;
    const double d0 = tj0 - ti0, d1 = tj1 - ti1, d2 = tj2 - ti2;
    r4[0] = (R00 * d0 + R10 * d1 + R20 * d2 - rec[0]) * w;
    r4[1] = (R01 * d0 + R11 * d1 + R21 * d2 - rec[1]) * w;
    r4[2] = (R02 * d0 + R12 * d1 + R22 * d2 - rec[2]) * w;
    r4[3] = sy_normalize(psi_j - psi_i - rec[3]) * w / 10.0;
    if (WANT_J) {
        const double k = w * (SY_PI / 180.0), w10 = w / 10.0;
        J1[0] = k * (R00 * d1 - R10 * d0); J1[1] = -w * R00; J1[2] = -w * R10; J1[3] = -w * R20;
        J1[4] = k * (R01 * d1 - R11 * d0); J1[5] = -w * R01; J1[6] = -w * R11; J1[7] = -w * R21;
        J1[8] = k * (R02 * d1 - R12 * d0); J1[9] = -w * R02; J1[10] = -w * R12; J1[11] = -w * R22;
        J1[12] = -w10; J1[13] = 0.0; J1[14] = 0.0; J1[15] = 0.0;
        J2[0] = 0.0; J2[1] = w * R00; J2[2] = w * R10; J2[3] = w * R20;
        J2[4] = 0.0; J2[5] = w * R01; J2[6] = w * R11; J2[7] = w * R21;
        J2[8] = 0.0; J2[9] = w * R02; J2[10] = w * R12; J2[11] = w * R22;
        J2[12] = w10; J2[13] = 0.0; J2[14] = 0.0; J2[15] = 0.0;
    }
}

// ---------------------------------------------------------------------------------------------
// The tables of a finalised graph and the arrays of one linearisation, as pointers — host or device.
// ---------------------------------------------------------------------------------------------
struct SyView {
    int64_t N, E;
    const int32_t* c1;          // [E] the edges' endpoints, add order
    const int32_t* c2;
    const double* edge_num;     // [E][SY_EDGE_DOUBLES]
    const uint8_t* node_free;   // [N]
    const int32_t* inc_ptr;     // [N + 1] a keyframe's incident list: (edge << 1) | side, add order
    const int32_t* inc;
};

// what a linearisation writes.  store: per edge J1[16] J2[16]
struct SyOut {
    double* residuals;      // [4 E]; may be NULL in a cost-only evaluation
    double* store;          // [E][32]
    double* offdiag;        // [E][36]
};

// the 6-wide slot of column k of a 4-wide block
#define SY_SLOT(k) ((k) == 0 ? 0 : (k) + 2)

// One edge.  Returns its cost term 0.5 |r|^2.  The 4 x 4 blocks live in registers: every index below is a compile-time one.
template <bool WANT_J>
PGO_HD double sy_block_item(const SyView& V, int64_t e, const double* quat, const double* t, const SyOut& O) {
    double r[4], J1[16], J2[16];
    const int64_t i = V.c1[e], j = V.c2[e];
    sy_residual<WANT_J>(quat[4 * i], t[3 * i], t[3 * i + 1], t[3 * i + 2], quat[4 * j], t[3 * j], t[3 * j + 1], t[3 * j + 2], V.edge_num + e * SY_EDGE_DOUBLES, r, J1, J2);
    double rho = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) rho += r[k] * r[k];
    if (O.residuals) {
#pragma unroll
        for (int k = 0; k < 4; ++k) O.residuals[4 * e + k] = r[k];
    }
    if (WANT_J) {
        double* s = O.store + e * 32;
#pragma unroll
        for (int k = 0; k < 16; ++k) { s[k] = J1[k]; s[16 + k] = J2[k]; }
        double* off = O.offdiag + e * 36;
#pragma unroll
        for (int k = 0; k < 36; ++k) off[k] = 0.0;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                double v = 0.0;
#pragma unroll
                for (int k = 0; k < 4; ++k) v += J1[k * 4 + a] * J2[k * 4 + b];
                off[SY_SLOT(a) * 6 + SY_SLOT(b)] = v;
            }
        }
    }
    return 0.5 * rho;
}

// H (upper triangle of 4 x 4, row-major in 16) += J^T J, g[4] += J^T r of one side of one edge, row by row
PGO_HD void sy_accumulate_side(const double* J, const double* r, double* H, double* g) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double j0 = J[k * 4], j1 = J[k * 4 + 1], j2 = J[k * 4 + 2], j3 = J[k * 4 + 3], rk = r[k];
        H[0] += j0 * j0; H[1] += j0 * j1; H[2] += j0 * j2; H[3] += j0 * j3;
        H[5] += j1 * j1; H[6] += j1 * j2; H[7] += j1 * j3;
        H[10] += j2 * j2; H[11] += j2 * j3;
        H[15] += j3 * j3;
        g[0] += j0 * rk; g[1] += j1 * rk; g[2] += j2 * rk; g[3] += j3 * rk;
    }
}

// One keyframe: diag [36] and grad [6] over its incident list in list order.  The upper triangle is summed and mirrored: the block is exactly symmetric.  Pad rows and
// columns are exactly 0, except diag[1][1] = diag[2][2] = 1 on a keyframe of the system (free and referenced by an edge): identity rows that keep the undamped matrix
// positive definite and give dpsi_pad = 0 in every step.  A constant keyframe, and a free one without an edge, gets zeros.
PGO_HD void sy_node_item(const SyView& V, int64_t node, const double* store, const double* residuals, double* diag, double* grad) {
    double H[16], g[4];
#pragma unroll
    for (int k = 0; k < 16; ++k) H[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) g[k] = 0.0;
    const int32_t k0 = V.inc_ptr[node], k1 = V.inc_ptr[node + 1];
    const bool in_system = V.node_free[node] && k1 > k0;
    if (in_system) {
        for (int32_t k = k0; k < k1; ++k) {
            const int64_t e = V.inc[k] >> 1;
            const int side = V.inc[k] & 1;
            sy_accumulate_side(store + e * 32 + side * 16, residuals + 4 * e, H, g);
        }
    }
    H[4] = H[1]; H[8] = H[2]; H[9] = H[6]; H[12] = H[3]; H[13] = H[7]; H[14] = H[11];
    double* D = diag + node * 36;
#pragma unroll
    for (int k = 0; k < 36; ++k) D[k] = 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
#pragma unroll
        for (int b = 0; b < 4; ++b) D[SY_SLOT(a) * 6 + SY_SLOT(b)] = H[a * 4 + b];
    }
    const double unit = in_system ? 1.0 : 0.0;
    D[7] = unit; D[14] = unit;
    double* G = grad + node * 6;
    G[0] = g[0]; G[1] = 0.0; G[2] = 0.0; G[3] = g[1]; G[4] = g[2]; G[5] = g[3];
}

// AngleLocalParameterization::Plus on the yaw slot, slots 1 - 3 copied, t + dt; t, t_out may be NULL
PGO_HD void sy_plus_item(int64_t i, const double* quat, const double* t, const double* delta, double* quat_out, double* t_out) {
    quat_out[4 * i] = sy_normalize(quat[4 * i] + delta[6 * i]);
    quat_out[4 * i + 1] = quat[4 * i + 1]; quat_out[4 * i + 2] = quat[4 * i + 2]; quat_out[4 * i + 3] = quat[4 * i + 3];
    if (t && t_out) { t_out[3 * i] = t[3 * i] + delta[6 * i + 3]; t_out[3 * i + 1] = t[3 * i + 1] + delta[6 * i + 4]; t_out[3 * i + 2] = t[3 * i + 2] + delta[6 * i + 5]; }
}

// ---------------------------------------------------------------------------------------------
// Host model
// ---------------------------------------------------------------------------------------------
// the binary tree of a workgroup's SY_CHUNK cost terms (v is overwritten): sg_block_kernel's
inline double sy_tree_sum(double* v) {
    for (int s = SY_CHUNK / 2; s >= 1; s >>= 1)
        for (int i = 0; i < s; ++i) v[i] = v[i] + v[i + s];
    return v[0];
}

struct SyGraph {
    int64_t N = 0;
    bool finalized = false;
    std::vector<int32_t> c1, c2, constant;
    std::vector<double> edge_num;
    // made by finalize
    std::vector<int32_t> inc_ptr, inc, pair_hi, pair_lo;
    std::vector<uint8_t> node_free, in_system;
    int64_t n_edges() const { return (int64_t)c1.size(); }

    int add_edges(int64_t n, const int32_t* a, const int32_t* b, const double* t_meas, const double* rel_yaw, const double* pitch, const double* roll, const double* weight, std::string& err) {
        if (finalized) { err = "edges added after pgo_sparse_yaw_graph_finalize"; return PGO_ERR_STATE; }
        if (n < 0 || (n > 0 && (!a || !b || !t_meas || !rel_yaw || !pitch || !roll))) { err = "null pointer or negative count"; return PGO_ERR_INVALID_ARG; }
        for (int64_t k = 0; k < n; ++k) {
            const std::string at = "edge " + std::to_string(k) + ": ";
            if (a[k] < 0 || a[k] >= N || b[k] < 0 || b[k] >= N) { err = at + "a keyframe out of range"; return PGO_ERR_INVALID_ARG; }
            if (a[k] == b[k]) { err = at + "an edge from a keyframe to itself"; return PGO_ERR_INVALID_ARG; }
            if (!std::isfinite(t_meas[3 * k]) || !std::isfinite(t_meas[3 * k + 1]) || !std::isfinite(t_meas[3 * k + 2]) || !std::isfinite(rel_yaw[k]) || !std::isfinite(pitch[k]) ||
                !std::isfinite(roll[k])) { err = at + "a non-finite number in the record"; return PGO_ERR_INVALID_ARG; }
            if (weight && !(std::isfinite(weight[k]) && weight[k] > 0.0)) { err = at + "the weight must be finite and > 0"; return PGO_ERR_INVALID_ARG; }
        }
        for (int64_t k = 0; k < n; ++k) {
            const double rec[SY_EDGE_DOUBLES] = {t_meas[3 * k], t_meas[3 * k + 1], t_meas[3 * k + 2], rel_yaw[k], pitch[k], roll[k], weight ? weight[k] : 1.0};
            c1.push_back(a[k]); c2.push_back(b[k]); edge_num.insert(edge_num.end(), rec, rec + SY_EDGE_DOUBLES);
        }
        return PGO_OK;
    }
    int set_constant(int64_t n, const int32_t* node, std::string& err) {
        if (finalized) { err = "constant keyframes set after pgo_sparse_yaw_graph_finalize"; return PGO_ERR_STATE; }
        if (n < 0 || (n > 0 && !node)) { err = "null pointer or negative count"; return PGO_ERR_INVALID_ARG; }
        for (int64_t k = 0; k < n; ++k) if (node[k] < 0 || node[k] >= N) { err = "constant keyframe " + std::to_string(k) + " out of range"; return PGO_ERR_INVALID_ARG; }
        constant.insert(constant.end(), node, node + n);
        return PGO_OK;
    }
    // the tables: the incident lists, free flags, the keyframes of the system (free and referenced by an edge), and the pair list of the factor — every pair of keyframes of
    // the system that an edge joins, once, sorted by (higher, lower)
    int finalize(std::string& err) {
        if (finalized) { err = "pgo_sparse_yaw_graph_finalize called twice"; return PGO_ERR_STATE; }
        const int64_t E = n_edges();
        if (E > (int64_t)(1 << 30) - 1) { err = "too many edges"; return PGO_ERR_INVALID_ARG; }
        std::vector<int32_t> count((size_t)N + 1, 0);
        for (int64_t e = 0; e < E; ++e) { ++count[(size_t)c1[(size_t)e] + 1]; ++count[(size_t)c2[(size_t)e] + 1]; }
        inc_ptr.assign((size_t)N + 1, 0);
        for (int64_t i = 0; i < N; ++i) inc_ptr[(size_t)i + 1] = inc_ptr[(size_t)i] + count[(size_t)i + 1];
        inc.assign((size_t)inc_ptr[(size_t)N], 0);
        std::vector<int32_t> fill(inc_ptr.begin(), inc_ptr.end() - 1);
        for (int64_t e = 0; e < E; ++e) { inc[(size_t)fill[(size_t)c1[(size_t)e]]++] = (int32_t)(e << 1); inc[(size_t)fill[(size_t)c2[(size_t)e]]++] = (int32_t)((e << 1) | 1); }
        node_free.assign((size_t)N, 1);
        for (int32_t n : constant) node_free[(size_t)n] = 0;
        in_system.assign((size_t)N, 0);
        for (int64_t i = 0; i < N; ++i) in_system[(size_t)i] = node_free[(size_t)i] && inc_ptr[(size_t)i + 1] > inc_ptr[(size_t)i] ? 1 : 0;
        std::vector<std::pair<int32_t, int32_t>> pr;
        for (int64_t e = 0; e < E; ++e) {
            const int32_t a = c1[(size_t)e], b = c2[(size_t)e];
            if (in_system[(size_t)a] && in_system[(size_t)b]) pr.emplace_back(a > b ? a : b, a > b ? b : a);
        }
        std::sort(pr.begin(), pr.end());
        pr.erase(std::unique(pr.begin(), pr.end()), pr.end());
        pair_hi.clear(); pair_lo.clear();
        for (const auto& p : pr) { pair_hi.push_back(p.first); pair_lo.push_back(p.second); }
        finalized = true;
        return PGO_OK;
    }
    SyView view() const { return SyView{N, n_edges(), c1.data(), c2.data(), edge_num.data(), node_free.data(), inc_ptr.data(), inc.data()}; }
    // what every evaluation checks of its arguments: the ambient layout keeps quat slots 1 - 3 exactly 0
    int check_state(const double* quat, const double* t, int64_t n_nodes, std::string& err) const {
        if (!finalized) { err = "the graph is evaluated before pgo_sparse_yaw_graph_finalize"; return PGO_ERR_STATE; }
        if (!quat || !t || n_nodes != N) { err = "null pointer, or n_nodes is not the graph's"; return PGO_ERR_INVALID_ARG; }
        for (int64_t i = 0; i < N; ++i)
            if (!(quat[4 * i + 1] == 0.0 && quat[4 * i + 2] == 0.0 && quat[4 * i + 3] == 0.0)) { err = "keyframe " + std::to_string(i) + ": quat slots 1 - 3 are not 0 (slot 0 holds the yaw in degrees)"; return PGO_ERR_INVALID_ARG; }
        return PGO_OK;
    }
};

// The serial instantiation: the same items in the same orders as the kernels of pgo_sparse_yaw.hpp.
struct SyHostLin {
    const SyGraph& G;
    std::vector<double> res, store, diag, grad, offdiag;
    bool linearised = false;
    explicit SyHostLin(const SyGraph& g) : G(g) {}
    template <bool WANT_J>
    double blocks(const SyView& V, const double* quat, const double* t, const SyOut& O) const {
        double total = 0.0, term[SY_CHUNK];
        for (int64_t e0 = 0; e0 < std::max<int64_t>(V.E, 1); e0 += SY_CHUNK) {
            for (int k = 0; k < SY_CHUNK; ++k) term[k] = e0 + k < V.E ? sy_block_item<WANT_J>(V, e0 + k, quat, t, O) : 0.0;
            total = total + sy_tree_sum(term);
        }
        return total;
    }
    int evaluate(const double* quat, const double* t, int64_t n_nodes, double* cost, double* residuals, double* gradient, std::string& err) {
        const int rc = G.check_state(quat, t, n_nodes, err);
        if (rc != PGO_OK) return rc;
        const SyView V = G.view();
        res.assign((size_t)V.E * 4, 0.0);
        double c;
        if (gradient) {
            store.assign((size_t)V.E * 32, 0.0); offdiag.assign((size_t)V.E * 36, 0.0); diag.assign((size_t)G.N * 36, 0.0); grad.assign((size_t)G.N * 6, 0.0);
            c = blocks<true>(V, quat, t, SyOut{res.data(), store.data(), offdiag.data()});
            for (int64_t i = 0; i < G.N; ++i) sy_node_item(V, i, store.data(), res.data(), diag.data(), grad.data());
            std::copy(grad.begin(), grad.end(), gradient);
            linearised = true;
        } else {
            c = blocks<false>(V, quat, t, SyOut{res.data(), nullptr, nullptr});
        }
        if (cost) *cost = c;
        if (residuals) std::copy(res.begin(), res.end(), residuals);
        return PGO_OK;
    }
    int normal_blocks(double* d, double* g, double* off, std::string& err) const {
        if (!linearised) { err = "no linearisation available (an evaluation with a gradient comes first)"; return PGO_ERR_STATE; }
        if (d) std::copy(diag.begin(), diag.end(), d);
        if (g) std::copy(grad.begin(), grad.end(), g);
        if (off) std::copy(offdiag.begin(), offdiag.end(), off);
        return PGO_OK;
    }
};

// J1, J2 [count][16] of edges first .. first + count - 1 out of a block store on the host
inline int sy_copy_jacobian_blocks(int64_t n_edges, const double* store, int64_t first, int64_t count, double* J1, double* J2, std::string& err) {
    if (first < 0 || count < 0 || first + count > n_edges) { err = "edges out of range"; return PGO_ERR_INVALID_ARG; }
    for (int64_t k = 0; k < count; ++k) {
        const double* s = store + (first + k) * 32;
        if (J1) std::copy(s, s + 16, J1 + k * 16);
        if (J2) std::copy(s + 16, s + 32, J2 + k * 16);
    }
    return PGO_OK;
}
}  // namespace pgo
