// pgo_sparse_graph_math.hpp — the linearisation of pgo_sparse_graph (include/pgo_sparse.h) per item, host and device (PGO_HD): what the kernels of
// pgo_sparse_graph.hpp run one thread per item and what a serial host instantiation (tests/native/sparse_graph_host.cpp) runs in a loop.  Plain C++: no HIP call.
//
//   switch_residual_ypr, switch_residual_ypr_robust   the reference's FourDOFErrorWithSwitchingConstraints (src/CeresResidues.h:338-422), composed of
//                                                     relpose_residual_ypr exactly as switch_residual composes relpose_residual;
//   sg_block_item       one residual block — relative-pose, switchable, regulariser — from the poses, its record and its switch: the residual, 0.5 rho, and with
//                       Jacobians J1, J2, dr/ds into the block store and J1^T J2, [J1^T Js ; J2^T Js], Js^T Js, Js^T r into their final places;
//   sg_node_item        a keyframe's diag and grad: J_side^T J_side and J_side^T r over its incident list in list order;
//   sg_plus_item        quat_plus and t + dt;
//   sg_tree_sum         the fixed binary tree a workgroup sums its cost terms by.
// SgGraph is the host model: the residual blocks as they were added, their validation (every PGO_ERR_INVALID_ARG of the interface), and the tables of _finalize.  Every
// address the items touch comes from these tables, none from the numbers.
//
// Orders (include/pgo.h): blocks = relative-pose edges in add order, switchable edges in add order, regularisers; residuals 6 / 7 / 6 per block in that order; the tangent
// layout [dtheta(3), dt(3)] per keyframe.  A robust block is the corrected one (Problem::Evaluate with apply_loss_function = true).
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

// ---------------------------------------------------------------------------------------------
// Switchable yaw/pitch/roll-weighted residual: with r6, A1, A2 = relpose_residual_ypr at w = 1 and the gains g (the reference multiplies all seven rows by s and
// ignores the weight, CeresResidues.h:397):
//   r = [ s r6 ; s (1 - s) ]   J1 = s A1, J2 = s A2 (7th row zero, not stored)   dr/ds = [ r6 ; 1 - 2 s ]
// ---------------------------------------------------------------------------------------------
template <bool WANT_J>
PGO_HD void switch_residual_ypr(const Pose& c1, const Pose& c2, const Meas& m, const double* g, double s, double* r7, double* J1, double* J2, double* Js7) {
    double r6[6];
    relpose_residual_ypr<WANT_J>(c1, c2, m, 1.0, g, r6, J1, J2);
#pragma unroll
    for (int i = 0; i < 6; ++i) r7[i] = s * r6[i];
    r7[6] = s * (1.0 - s);
    if (WANT_J) {
#pragma unroll
        for (int i = 0; i < 36; ++i) { J1[i] *= s; J2[i] *= s; }
#pragma unroll
        for (int i = 0; i < 6; ++i) Js7[i] = r6[i];
        Js7[6] = 1.0 - 2.0 * s;
    }
}

// ... under the loss `enc`, as switch_residual_robust: s_hat over all SEVEN rows, c = sqrt(rho'(s_hat)) scales r and all five blocks; enc = 0 gives c = 1 and the bits of
// switch_residual_ypr.  Returns rho(s_hat).
template <bool WANT_J>
PGO_HD double switch_residual_ypr_robust(const Pose& c1, const Pose& c2, const Meas& m, const double* g, double s, double enc, double* r7, double* J1, double* J2, double* Js7, double& c) {
    double r0[6];
    relpose_residual_ypr<false>(c1, c2, m, 1.0, g, r0, nullptr, nullptr);
    const double p = s * (1.0 - s);
    double sh = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) { const double v = s * r0[i]; sh += v * v; }
    sh += p * p;
    const double rho = robust_loss(enc, sh, c);
    double r6[6];
    relpose_residual_ypr<WANT_J>(c1, c2, m, 1.0, g, r6, J1, J2);
#pragma unroll
    for (int i = 0; i < 6; ++i) r7[i] = c * (s * r6[i]);
    r7[6] = c * p;
    if (WANT_J) {
        const double cs = c * s;
#pragma unroll
        for (int i = 0; i < 36; ++i) { J1[i] *= cs; J2[i] *= cs; }
#pragma unroll
        for (int i = 0; i < 6; ++i) Js7[i] = c * r6[i];
        Js7[6] = c * (1.0 - 2.0 * s);
    }
    return rho;
}

// ---------------------------------------------------------------------------------------------
// The per-block products.  Every sum runs over the residual rows in ascending order.
// ---------------------------------------------------------------------------------------------
// out[36] = A^T B of two 6 x 6 row-major blocks
PGO_HD void sg_atb(const double* A, const double* B, double* out) {
#pragma unroll
    for (int a = 0; a < 6; ++a) {
#pragma unroll
        for (int b = 0; b < 6; ++b) {
            double s = 0.0;
#pragma unroll
            for (int i = 0; i < 6; ++i) s += A[i * 6 + a] * B[i * 6 + b];
            out[a * 6 + b] = s;
        }
    }
}
// out[6] = A^T v (the six rows A has)
PGO_HD void sg_atv(const double* A, const double* v, double* out) {
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < 6; ++i) s += A[i * 6 + a] * v[i];
        out[a] = s;
    }
}
PGO_HD double sg_dot7(const double* a, const double* b) {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 7; ++i) s += a[i] * b[i];
    return s;
}
// H[36] += J^T J, g[6] += J^T r of one side of one block, row by row: only the upper triangle is summed and then mirrored by the caller (sg_mirror), so a diagonal block is
// exactly symmetric.  J [36] row-major, r the block's first six residuals (a switchable block's 7th row of J is zero).
PGO_HD void sg_accumulate_side(const double* J, const double* r, double* H, double* g) {
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const double j0 = J[i * 6], j1 = J[i * 6 + 1], j2 = J[i * 6 + 2], j3 = J[i * 6 + 3], j4 = J[i * 6 + 4], j5 = J[i * 6 + 5], ri = r[i];
        H[0] += j0 * j0; H[1] += j0 * j1; H[2] += j0 * j2; H[3] += j0 * j3; H[4] += j0 * j4; H[5] += j0 * j5;
        H[7] += j1 * j1; H[8] += j1 * j2; H[9] += j1 * j3; H[10] += j1 * j4; H[11] += j1 * j5;
        H[14] += j2 * j2; H[15] += j2 * j3; H[16] += j2 * j4; H[17] += j2 * j5;
        H[21] += j3 * j3; H[22] += j3 * j4; H[23] += j3 * j5;
        H[28] += j4 * j4; H[29] += j4 * j5;
        H[35] += j5 * j5;
        g[0] += j0 * ri; g[1] += j1 * ri; g[2] += j2 * ri; g[3] += j3 * ri; g[4] += j4 * ri; g[5] += j5 * ri;
    }
}
PGO_HD void sg_mirror(double* H) {
    H[6] = H[1]; H[12] = H[2]; H[13] = H[8]; H[18] = H[3]; H[19] = H[9]; H[20] = H[15];
    H[24] = H[4]; H[25] = H[10]; H[26] = H[16]; H[27] = H[22]; H[30] = H[5]; H[31] = H[11]; H[32] = H[17]; H[33] = H[23]; H[34] = H[29];
}

// ---------------------------------------------------------------------------------------------
// The tables of a finalised graph and the arrays of one linearisation, as pointers — host or device.
// ---------------------------------------------------------------------------------------------
constexpr int SG_EDGE_DOUBLES = 12;      // q_obs[4] t_obs[3] w | gains[3] | loss (+a Huber, -a Cauchy, 0 trivial)
constexpr int SG_PRIOR_DOUBLES = 17;     // Rf[9] tf[3] qf[4] w
constexpr int SG_CHUNK = 256;            // cost terms per partial sum: a workgroup of the block kernel

struct SgView {
    int64_t N, n_rel, n_sw, n_prior;
    const int32_t* c1;          // [n_rel + n_sw] the edges' endpoints, internal order
    const int32_t* c2;
    const int32_t* sw_index;    // [n_sw]
    const int32_t* prior_node;  // [n_prior]
    const double* edge_num;     // [n_rel + n_sw][SG_EDGE_DOUBLES]
    const double* prior_num;    // [n_prior][SG_PRIOR_DOUBLES]
    const uint8_t* node_free;   // [N]
    const int32_t* inc_ptr;     // [N + 1] a keyframe's incident list: (block << 1) | side, internal edge order, regularisers last
    const int32_t* inc;
    PGO_HD int64_t blocks() const { return n_rel + n_sw + n_prior; }
    PGO_HD int64_t residuals() const { return 6 * n_rel + 7 * n_sw + 6 * n_prior; }
    PGO_HD int64_t residual_at(int64_t b) const { return b < n_rel ? 6 * b : b < n_rel + n_sw ? 6 * n_rel + 7 * (b - n_rel) : 6 * n_rel + 7 * n_sw + 6 * (b - n_rel - n_sw); }
};

// what a linearisation writes.  store: per block J1[36] J2[36] (a regulariser: J1 alone, J2 zeros); r is the residual array itself (pgo_evaluate's order)
struct SgOut {
    double* residuals;      // [V.residuals()]; may be NULL in a cost-only evaluation
    double* store;          // [blocks][72]
    double* dr_ds;          // [n_sw][7]
    double* offdiag;        // [n_rel + n_sw][36]
    double* sw_c;           // [n_sw][12]
    double* sw_hss;         // [n_sw]
    double* sw_gs;          // [n_sw]
};

PGO_HD Pose sg_pose(const double* quat, const double* t, int64_t i) {
    return Pose{quat[4 * i], quat[4 * i + 1], quat[4 * i + 2], quat[4 * i + 3], t[3 * i], t[3 * i + 1], t[3 * i + 2]};
}

// One residual block.  Returns its cost term 0.5 rho.  YPR / LOSS: the graph has a yaw/pitch/roll-weighted / a robust edge at all — a graph without pays for neither (the
// three atan2, the second evaluation); inside, the edge's own record decides.  The 6 x 6 blocks live in registers: every index below is a compile-time one.
template <bool WANT_J, bool YPR, bool LOSS>
PGO_HD double sg_block_item(const SgView& V, int64_t b, const double* quat, const double* t, const double* sw, const SgOut& O) {
    double r[7], J1[36], J2[36], Js[7];
    double rho;
    const int64_t at = V.residual_at(b);
    if (b >= V.n_rel + V.n_sw) {      // a regulariser
        const int64_t k = b - V.n_rel - V.n_sw;
        const double* p = V.prior_num + k * SG_PRIOR_DOUBLES;
        const Pose c = sg_pose(quat, t, V.prior_node[k]);
        prior_residual<WANT_J>(c, p, p + 9, p + 12, p[16], r, J1);
        rho = 0.0;
#pragma unroll
        for (int i = 0; i < 6; ++i) rho += r[i] * r[i];
        if (O.residuals) {
#pragma unroll
            for (int i = 0; i < 6; ++i) O.residuals[at + i] = r[i];
        }
        if (WANT_J) {
            double* s1 = O.store + b * 72;
#pragma unroll
            for (int i = 0; i < 36; ++i) { s1[i] = J1[i]; s1[36 + i] = 0.0; }
        }
        return 0.5 * rho;
    }
    const double* e = V.edge_num + b * SG_EDGE_DOUBLES;
    const Meas m{e[0], e[1], e[2], e[3], e[4], e[5], e[6], e[7]};
    const double g[3] = {e[8], e[9], e[10]};
    const double enc = e[11];
    const Pose p1 = sg_pose(quat, t, V.c1[b]), p2 = sg_pose(quat, t, V.c2[b]);
    const bool ypr = YPR && g[0] > 0.0;
    const bool is_sw = b >= V.n_rel;
    double c;
    if (!is_sw) {
        if (LOSS && enc != 0.0) {
            rho = ypr ? relpose_residual_ypr_robust<WANT_J>(p1, p2, m, g, enc, r, J1, J2, c) : relpose_residual_robust<WANT_J>(p1, p2, m, enc, r, J1, J2, c);
        } else {
            if (ypr) relpose_residual_ypr<WANT_J>(p1, p2, m, m.w, g, r, J1, J2); else relpose_residual<WANT_J>(p1, p2, m, m.w, r, J1, J2);
            rho = 0.0;
#pragma unroll
            for (int i = 0; i < 6; ++i) rho += r[i] * r[i];
        }
    } else {
        const double s = sw[V.sw_index[b - V.n_rel]];
        if (LOSS && enc != 0.0) {
            rho = ypr ? switch_residual_ypr_robust<WANT_J>(p1, p2, m, g, s, enc, r, J1, J2, Js, c) : switch_residual_robust<WANT_J>(p1, p2, m, s, enc, r, J1, J2, Js, c);
        } else {
            if (ypr) switch_residual_ypr<WANT_J>(p1, p2, m, g, s, r, J1, J2, Js); else switch_residual<WANT_J>(p1, p2, m, s, r, J1, J2, Js);
            rho = 0.0;
#pragma unroll
            for (int i = 0; i < 7; ++i) rho += r[i] * r[i];
        }
    }
    if (O.residuals) {
#pragma unroll
        for (int i = 0; i < 6; ++i) O.residuals[at + i] = r[i];
        if (is_sw) O.residuals[at + 6] = r[6];
    }
    if (WANT_J) {
        double* s1 = O.store + b * 72;
#pragma unroll
        for (int i = 0; i < 36; ++i) { s1[i] = J1[i]; s1[36 + i] = J2[i]; }
        sg_atb(J1, J2, O.offdiag + b * 36);
        if (is_sw) {
            const int64_t k = b - V.n_rel;
            double v[6];
            sg_atv(J1, Js, v);
#pragma unroll
            for (int i = 0; i < 6; ++i) O.sw_c[k * 12 + i] = v[i];
            sg_atv(J2, Js, v);
#pragma unroll
            for (int i = 0; i < 6; ++i) O.sw_c[k * 12 + 6 + i] = v[i];
#pragma unroll
            for (int i = 0; i < 7; ++i) O.dr_ds[k * 7 + i] = Js[i];
            O.sw_hss[k] = sg_dot7(Js, Js);
            O.sw_gs[k] = sg_dot7(Js, r);
        }
    }
    return 0.5 * rho;
}

// One keyframe: diag [36] and grad [6] over its incident list in list order; a constant keyframe gets zeros.  residuals: the array the block items wrote.
PGO_HD void sg_node_item(const SgView& V, int64_t node, const double* store, const double* residuals, double* diag, double* grad) {
    double H[36], g[6];
#pragma unroll
    for (int i = 0; i < 36; ++i) H[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) g[i] = 0.0;
    if (V.node_free[node]) {
        for (int32_t k = V.inc_ptr[node]; k < V.inc_ptr[node + 1]; ++k) {
            const int64_t b = V.inc[k] >> 1;
            const int side = V.inc[k] & 1;
            sg_accumulate_side(store + b * 72 + side * 36, residuals + V.residual_at(b), H, g);
        }
        sg_mirror(H);
    }
#pragma unroll
    for (int i = 0; i < 36; ++i) diag[node * 36 + i] = H[i];
#pragma unroll
    for (int i = 0; i < 6; ++i) grad[node * 6 + i] = g[i];
}

// ceres::EigenQuaternionParameterization::Plus and t + dt of one keyframe; t, t_out may be NULL
PGO_HD void sg_plus_item(int64_t i, const double* quat, const double* t, const double* delta, double* quat_out, double* t_out) {
    // quat_plus' expressions on scalars (quat_mul(dq, q)): its arrays behind a branch would live in scratch
    const double q0 = quat[4 * i], q1 = quat[4 * i + 1], q2 = quat[4 * i + 2], q3 = quat[4 * i + 3];
    const double d0 = delta[6 * i], d1 = delta[6 * i + 1], d2 = delta[6 * i + 2];
    const double n = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
    double o0 = q0, o1 = q1, o2 = q2, o3 = q3;
    if (n > 0.0) {
        const double sbd = sin(n) / n;
        const double a0 = sbd * d0, a1 = sbd * d1, a2 = sbd * d2, a3 = cos(n);
        o3 = a3 * q3 - a0 * q0 - a1 * q1 - a2 * q2;
        o0 = a3 * q0 + a0 * q3 + a1 * q2 - a2 * q1;
        o1 = a3 * q1 + a1 * q3 + a2 * q0 - a0 * q2;
        o2 = a3 * q2 + a2 * q3 + a0 * q1 - a1 * q0;
    }
    quat_out[4 * i] = o0; quat_out[4 * i + 1] = o1; quat_out[4 * i + 2] = o2; quat_out[4 * i + 3] = o3;
    if (t && t_out) { t_out[3 * i] = t[3 * i] + delta[6 * i + 3]; t_out[3 * i + 1] = t[3 * i + 1] + delta[6 * i + 4]; t_out[3 * i + 2] = t[3 * i + 2] + delta[6 * i + 5]; }
}

// ---------------------------------------------------------------------------------------------
// Host model
// ---------------------------------------------------------------------------------------------
// the binary tree of a workgroup's SG_CHUNK cost terms (v is overwritten): step s adds v[i + s] into v[i] for i < s, s = 128, 64, ..., 1
inline double sg_tree_sum(double* v) {
    for (int s = SG_CHUNK / 2; s >= 1; s >>= 1)
        for (int i = 0; i < s; ++i) v[i] = v[i] + v[i + s];
    return v[0];
}

struct SgGraph {
    int64_t N = 0;
    bool finalized = false;
    bool any_ypr = false, any_loss = false;
    std::vector<int32_t> rel_c1, rel_c2, sw_c1, sw_c2, sw_idx, prior_node, constant;
    std::vector<double> rel_num, sw_num, prior_num;
    // made by finalize
    std::vector<int32_t> c1, c2, inc_ptr, inc, pair_hi, pair_lo;
    std::vector<double> edge_num;
    std::vector<uint8_t> node_free, in_system;
    int64_t n_rel() const { return (int64_t)rel_c1.size(); }
    int64_t n_sw() const { return (int64_t)sw_c1.size(); }
    int64_t n_prior() const { return (int64_t)prior_node.size(); }
    int64_t min_switches() const { int32_t m = -1; for (int32_t s : sw_idx) m = s > m ? s : m; return (int64_t)m + 1; }

    static void meas(const double* T, double w, double* out8) {      // Matrix4d (column-major 16) -> q_obs (Eigen's Matrix3 -> Quaternion rule), t_obs, weight
        double R[9], q[4];
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) R[r * 3 + c] = T[c * 4 + r];
        eigen_matrix_to_quat(R, q);
        out8[0] = q[0]; out8[1] = q[1]; out8[2] = q[2]; out8[3] = q[3];
        out8[4] = T[12]; out8[5] = T[13]; out8[6] = T[14]; out8[7] = w;
    }
    // what both add calls refuse; the text of the first fault, or empty
    std::string check_edges(int64_t n, const int32_t* a, const int32_t* b, const double* T, const double* w, const double* gains, int32_t loss, double loss_a) const {
        if (n < 0 || (n > 0 && (!a || !b || !T))) return "null pointer or negative count";
        if (loss != PGO_LOSS_TRIVIAL && loss != PGO_LOSS_HUBER && loss != PGO_LOSS_CAUCHY) return "unknown robust loss";
        if (loss != PGO_LOSS_TRIVIAL && !(std::isfinite(loss_a) && loss_a > 0.0)) return "the robust loss parameter must be finite and positive";
        for (int64_t k = 0; k < n; ++k) {
            const std::string at = "edge " + std::to_string(k) + ": ";
            if (a[k] < 0 || a[k] >= N || b[k] < 0 || b[k] >= N) return at + "a keyframe out of range";
            if (a[k] == b[k]) return at + "an edge from a keyframe to itself";
            for (int i = 0; i < 16; ++i) if (!std::isfinite(T[16 * k + i])) return at + "a non-finite measurement";
            if (w && !std::isfinite(w[k])) return at + "a non-finite weight";
            if (gains) {
                const double* g = gains + 3 * k;
                const bool zero = g[0] == 0.0 && g[1] == 0.0 && g[2] == 0.0;
                const bool pos = std::isfinite(g[0]) && std::isfinite(g[1]) && std::isfinite(g[2]) && g[0] > 0.0 && g[1] > 0.0 && g[2] > 0.0;
                if (!zero && !pos) return at + "yaw/pitch/roll gains must be all zero or all > 0 and finite";
            }
        }
        return "";
    }
    void push_edges(std::vector<int32_t>& e1, std::vector<int32_t>& e2, std::vector<double>& num, int64_t n, const int32_t* a, const int32_t* b, const double* T, const double* w, const double* gains,
                    int32_t loss, double loss_a) {
        const double enc = loss == PGO_LOSS_HUBER ? loss_a : loss == PGO_LOSS_CAUCHY ? -loss_a : 0.0;
        for (int64_t k = 0; k < n; ++k) {
            double rec[SG_EDGE_DOUBLES];
            meas(T + 16 * k, w ? w[k] : 1.0, rec);
            for (int i = 0; i < 3; ++i) rec[8 + i] = gains ? gains[3 * k + i] : 0.0;
            rec[11] = enc;
            if (rec[8] > 0.0) any_ypr = true;
            if (enc != 0.0) any_loss = true;
            e1.push_back(a[k]); e2.push_back(b[k]); num.insert(num.end(), rec, rec + SG_EDGE_DOUBLES);
        }
    }
    int add_relpose(int64_t n, const int32_t* a, const int32_t* b, const double* T, const double* w, const double* gains, int32_t loss, double loss_a, std::string& err) {
        if (finalized) { err = "edges added after pgo_sparse_graph_finalize"; return PGO_ERR_STATE; }
        if (n > 0 && !w) { err = "weight array required for relative-pose edges"; return PGO_ERR_INVALID_ARG; }
        err = check_edges(n, a, b, T, w, gains, loss, loss_a);
        if (!err.empty()) return PGO_ERR_INVALID_ARG;
        push_edges(rel_c1, rel_c2, rel_num, n, a, b, T, w, gains, loss, loss_a);
        return PGO_OK;
    }
    int add_switchable(int64_t n, const int32_t* a, const int32_t* b, const double* T, const int32_t* idx, const double* gains, int32_t loss, double loss_a, std::string& err) {
        if (finalized) { err = "edges added after pgo_sparse_graph_finalize"; return PGO_ERR_STATE; }
        if (n > 0 && !idx) { err = "switch index array required"; return PGO_ERR_INVALID_ARG; }
        err = check_edges(n, a, b, T, nullptr, gains, loss, loss_a);
        if (!err.empty()) return PGO_ERR_INVALID_ARG;
        std::vector<int32_t> seen(sw_idx);
        for (int64_t k = 0; k < n; ++k) {
            if (idx[k] < 0) { err = "edge " + std::to_string(k) + ": a negative switch index"; return PGO_ERR_INVALID_ARG; }
            for (int32_t s : seen) if (s == idx[k]) { err = "edge " + std::to_string(k) + ": a switch index used twice"; return PGO_ERR_INVALID_ARG; }
            seen.push_back(idx[k]);
        }
        push_edges(sw_c1, sw_c2, sw_num, n, a, b, T, nullptr, gains, loss, loss_a);
        sw_idx.insert(sw_idx.end(), idx, idx + n);
        return PGO_OK;
    }
    // REPLACES the regulariser set (pgo_set_node_regularizers)
    int set_priors(int64_t n, const int32_t* node, const double* target, const double* weight, std::string& err) {
        if (finalized) { err = "regularisers set after pgo_sparse_graph_finalize"; return PGO_ERR_STATE; }
        if (n < 0 || (n > 0 && (!node || !target || !weight))) { err = "null pointer or negative count"; return PGO_ERR_INVALID_ARG; }
        for (int64_t k = 0; k < n; ++k) {
            if (node[k] < 0 || node[k] >= N) { err = "regulariser " + std::to_string(k) + ": a keyframe out of range"; return PGO_ERR_INVALID_ARG; }
            for (int i = 0; i < 16; ++i) if (!std::isfinite(target[16 * k + i])) { err = "regulariser " + std::to_string(k) + ": a non-finite target"; return PGO_ERR_INVALID_ARG; }
            if (!std::isfinite(weight[k])) { err = "regulariser " + std::to_string(k) + ": a non-finite weight"; return PGO_ERR_INVALID_ARG; }
        }
        prior_node.assign(node, node + n);
        prior_num.assign((size_t)n * SG_PRIOR_DOUBLES, 0.0);
        for (int64_t k = 0; k < n; ++k) {
            double* p = &prior_num[(size_t)k * SG_PRIOR_DOUBLES];
            const double* T = target + 16 * k;
            for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) p[r * 3 + c] = T[c * 4 + r];
            p[9] = T[12]; p[10] = T[13]; p[11] = T[14];
            eigen_matrix_to_quat(p, p + 12);
            p[16] = weight[k];
        }
        return PGO_OK;
    }
    int set_constant(int64_t n, const int32_t* node, std::string& err) {
        if (finalized) { err = "constant keyframes set after pgo_sparse_graph_finalize"; return PGO_ERR_STATE; }
        if (n < 0 || (n > 0 && !node)) { err = "null pointer or negative count"; return PGO_ERR_INVALID_ARG; }
        for (int64_t k = 0; k < n; ++k) if (node[k] < 0 || node[k] >= N) { err = "constant keyframe " + std::to_string(k) + " out of range"; return PGO_ERR_INVALID_ARG; }
        constant.insert(constant.end(), node, node + n);
        return PGO_OK;
    }
    // the tables: the edges in internal order, the incident lists, free flags (a keyframe no block references is not free of anything: it is outside the system), and the
    // pair list of the factor — every pair of keyframes of the system that an edge joins, once, sorted by (higher, lower)
    int finalize(std::string& err) {
        if (finalized) { err = "pgo_sparse_graph_finalize called twice"; return PGO_ERR_STATE; }
        const int64_t Er = n_rel(), Es = n_sw(), Eg = n_prior();
        if ((Er + Es + Eg) > (int64_t)(1 << 30) - 1) { err = "too many residual blocks"; return PGO_ERR_INVALID_ARG; }
        c1 = rel_c1; c1.insert(c1.end(), sw_c1.begin(), sw_c1.end());
        c2 = rel_c2; c2.insert(c2.end(), sw_c2.begin(), sw_c2.end());
        edge_num = rel_num; edge_num.insert(edge_num.end(), sw_num.begin(), sw_num.end());
        std::vector<int32_t> count((size_t)N + 1, 0);
        for (int64_t e = 0; e < Er + Es; ++e) { ++count[(size_t)c1[(size_t)e] + 1]; ++count[(size_t)c2[(size_t)e] + 1]; }
        for (int32_t n : prior_node) ++count[(size_t)n + 1];
        inc_ptr.assign((size_t)N + 1, 0);
        for (int64_t i = 0; i < N; ++i) inc_ptr[(size_t)i + 1] = inc_ptr[(size_t)i] + count[(size_t)i + 1];
        inc.assign((size_t)inc_ptr[(size_t)N], 0);
        std::vector<int32_t> fill(inc_ptr.begin(), inc_ptr.end() - 1);
        for (int64_t e = 0; e < Er + Es; ++e) { inc[(size_t)fill[(size_t)c1[(size_t)e]]++] = (int32_t)(e << 1); inc[(size_t)fill[(size_t)c2[(size_t)e]]++] = (int32_t)((e << 1) | 1); }
        for (int64_t k = 0; k < Eg; ++k) inc[(size_t)fill[(size_t)prior_node[(size_t)k]]++] = (int32_t)((Er + Es + k) << 1);
        node_free.assign((size_t)N, 1);
        for (int32_t n : constant) node_free[(size_t)n] = 0;
        in_system.assign((size_t)N, 0);
        for (int64_t i = 0; i < N; ++i) in_system[(size_t)i] = node_free[(size_t)i] && inc_ptr[(size_t)i + 1] > inc_ptr[(size_t)i] ? 1 : 0;
        std::vector<std::pair<int32_t, int32_t>> pr;
        for (int64_t e = 0; e < Er + Es; ++e) {
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
    SgView view() const {      // over the host tables
        return SgView{N, n_rel(), n_sw(), n_prior(), c1.data(), c2.data(), sw_idx.data(), prior_node.data(), edge_num.data(), prior_num.data(), node_free.data(), inc_ptr.data(), inc.data()};
    }
    // what every evaluation checks of its arguments
    int check_state(const double* quat, const double* t, const double* sw, int64_t n_nodes, int64_t n_switch, std::string& err) const {
        if (!finalized) { err = "the graph is evaluated before pgo_sparse_graph_finalize"; return PGO_ERR_STATE; }
        if (!quat || !t || n_nodes != N || n_switch < min_switches() || (n_switch > 0 && !sw)) { err = "null pointer, n_nodes is not the graph's, or n_switch below a switch index in use"; return PGO_ERR_INVALID_ARG; }
        return PGO_OK;
    }
};

// The serial instantiation: the same items in the same orders as the kernels of pgo_sparse_graph.hpp.
struct SgHostLin {
    const SgGraph& G;
    std::vector<double> res, store, dr_ds, diag, grad, offdiag, sw_c, sw_hss, sw_gs;
    bool linearised = false;
    explicit SgHostLin(const SgGraph& g) : G(g) {}
    template <bool WANT_J>
    double blocks(const SgView& V, const double* quat, const double* t, const double* sw, const SgOut& O) const {
        const int64_t B = V.blocks();
        double total = 0.0, term[SG_CHUNK];
        for (int64_t b0 = 0; b0 < B; b0 += SG_CHUNK) {
            for (int k = 0; k < SG_CHUNK; ++k) {
                const int64_t b = b0 + k;
                term[k] = b >= B ? 0.0
                        : G.any_ypr ? (G.any_loss ? sg_block_item<WANT_J, true, true>(V, b, quat, t, sw, O) : sg_block_item<WANT_J, true, false>(V, b, quat, t, sw, O))
                                    : (G.any_loss ? sg_block_item<WANT_J, false, true>(V, b, quat, t, sw, O) : sg_block_item<WANT_J, false, false>(V, b, quat, t, sw, O));
            }
            total = total + sg_tree_sum(term);
        }
        return total;
    }
    int evaluate(const double* quat, const double* t, const double* sw, int64_t n_nodes, int64_t n_switch, double* cost, double* residuals, double* gradient, std::string& err) {
        const int rc = G.check_state(quat, t, sw, n_nodes, n_switch, err);
        if (rc != PGO_OK) return rc;
        const SgView V = G.view();
        const size_t E = (size_t)(V.n_rel + V.n_sw), Es = (size_t)V.n_sw;
        res.assign((size_t)V.residuals(), 0.0);
        double c;
        if (gradient) {
            store.assign((size_t)V.blocks() * 72, 0.0); dr_ds.assign(Es * 7, 0.0); offdiag.assign(E * 36, 0.0); sw_c.assign(Es * 12, 0.0); sw_hss.assign(Es, 0.0); sw_gs.assign(Es, 0.0);
            diag.assign((size_t)G.N * 36, 0.0); grad.assign((size_t)G.N * 6, 0.0);
            const SgOut O{res.data(), store.data(), dr_ds.data(), offdiag.data(), sw_c.data(), sw_hss.data(), sw_gs.data()};
            c = blocks<true>(V, quat, t, sw, O);
            for (int64_t i = 0; i < G.N; ++i) sg_node_item(V, i, store.data(), res.data(), diag.data(), grad.data());
            std::copy(grad.begin(), grad.end(), gradient);
            for (int64_t i = 0; i < n_switch; ++i) gradient[6 * G.N + i] = 0.0;
            for (size_t e = 0; e < Es; ++e) gradient[6 * G.N + G.sw_idx[e]] = sw_gs[e];
            linearised = true;
        } else {
            const SgOut O{res.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
            c = blocks<false>(V, quat, t, sw, O);
        }
        if (cost) *cost = c;
        if (residuals) std::copy(res.begin(), res.end(), residuals);
        return PGO_OK;
    }
    int normal_blocks(double* d, double* g, double* off, double* c, double* hss, double* gs, std::string& err) const {
        if (!linearised) { err = "no linearisation available (an evaluation with a gradient comes first)"; return PGO_ERR_STATE; }
        if (d) std::copy(diag.begin(), diag.end(), d);
        if (g) std::copy(grad.begin(), grad.end(), g);
        if (off) std::copy(offdiag.begin(), offdiag.end(), off);
        if (c) std::copy(sw_c.begin(), sw_c.end(), c);
        if (hss) std::copy(sw_hss.begin(), sw_hss.end(), hss);
        if (gs) std::copy(sw_gs.begin(), sw_gs.end(), gs);
        return PGO_OK;
    }
};

// pgo_get_jacobian_blocks' contract over a block store and dr/ds array on the host: kind 0 relative-pose, 1 switchable, 2 regulariser
inline int sg_copy_jacobian_blocks(const SgGraph& G, const double* store, const double* dr, int32_t kind, int64_t first, int64_t count, double* J1, double* J2, double* dr_ds, std::string& err) {
    if (kind < 0 || kind > 2 || first < 0 || count < 0) { err = "unknown kind or negative range"; return PGO_ERR_INVALID_ARG; }
    const int64_t n = kind == 0 ? G.n_rel() : kind == 1 ? G.n_sw() : G.n_prior();
    if (first + count > n) { err = "blocks out of range"; return PGO_ERR_INVALID_ARG; }
    const int64_t b0 = (kind == 0 ? 0 : kind == 1 ? G.n_rel() : G.n_rel() + G.n_sw()) + first;
    for (int64_t k = 0; k < count; ++k) {
        const double* s = store + (b0 + k) * 72;
        if (J1) std::copy(s, s + 36, J1 + k * 36);
        if (J2 && kind != 2) std::copy(s + 36, s + 72, J2 + k * 36);
        if (dr_ds && kind == 1) std::copy(dr + (first + k) * 7, dr + (first + k) * 7 + 7, dr_ds + k * 7);
    }
    return PGO_OK;
}
}  // namespace pgo
