// pgo_dense_math.hpp — the arithmetic of the dense Cholesky solver (pgo_dense.hip) that does not need a GPU: the factorisation of one 64 x 64 diagonal block, the two
// triangular solves with such a block, the order of the block steps, and a serial host instantiation of the whole blocked factor and solve on the same order of operations
// (tests/native/dense_chol_host.cpp).  The block routines are written once for a TEAM of cooperating threads: rank() / size() / sync().  The kernels pass their workgroup
// (256 threads, sync = __syncthreads), the host passes DcSerial (one thread, no barrier): every entry sees the same operations in the same order on both.
//
// The algorithm: blocked right-looking Cholesky A = L L^T on the LOWER triangle of a row-major n x n matrix, n a multiple of 64, in place.  Per block step k
//   panel   L_ik = A_ik L_kk^-T for every tile row i > k — a true triangular substitution, never a product with an inverse, so the factor is backward stable
//           whatever the conditioning of L_kk;
//   update  A_ij -= L_ik L_jk^T for k < j <= i, and the diagonal tile (k + 1, k + 1) is factored as soon as it has been updated.
// Solve: L y = b by block columns (y_k = L_kk^-1 w_k, then w_i -= L_ik y_k for i > k), L^T x = y by block rows from the bottom (x_k = L_kk^-T y_k, then
// y_j -= L_kj^T x_k for j < k).  Every sum has a fixed order: two runs give the same bits.
//
// Covariance blocks (pgo_pose_covariance, pgo_covariance): Sigma = (L L^T)^-1 = L^-T L^-1, so the 6 x 6 block of keyframes (a, b) is (L^-1 E_a)^T (L^-1 E_b) with E_c the 6 unit columns of
// keyframe c: forward substitutions only.  The right-hand sides are the ROWS of W (m x n row-major, m a multiple of 64, sorted by the column of their one), solved in place
// by block columns k:   solve  Y = W_.k L_kk^-T for every 64-row tile of W (the panel's substitution);   update  W_.i -= Y L_ik^T for i > k.
// A unit column is zero before its one, so a tile row of W whose first right-hand side starts in tile k0 has nothing but zeros to solve and to subtract in the steps k < k0:
// they are skipped (dc_cov_steps), and since every skipped operation would have produced or subtracted +0 the result has the same bits with and without the skipping.
// Then   gram  Sigma_ab = W_a W_b^T over the n columns (dc_param_gram_block): 256 column classes (column mod 256) summed ascending, then a fixed binary tree over the classes —
// the same operations whatever the size of the team, and the same for (a, b) and (b, a) with the factors of every product swapped: the block of (b, a) is the exact transpose.
// Switch parameters (pgo_covariance) add one right-hand-side row each and Gram products of 6- and 1-row blocks; a matrix-free handle's matrix is assembled from its normal
// blocks: both further down, with their plans.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <vector>

#if defined(__HIPCC__)
#define PGO_DC_HD __host__ __device__ __forceinline__
#else
#define PGO_DC_HD inline
#endif

namespace pgo {

constexpr int DC_NB = 64;           // block size = tile size
constexpr int DC_LD = DC_NB + 1;    // row stride of a block held in LDS (conflict-free column walks)
constexpr int DC_SUB = 16;          // the panel's substitution works on 16 x 16 sub-blocks (one MFMA tile)

struct DcSerial {
    PGO_DC_HD int rank() const { return 0; }
    PGO_DC_HD int size() const { return 1; }
    PGO_DC_HD void sync() const {}
};

// the pivot test of gj_block_inverse: not positive, or NaN
PGO_DC_HD bool dc_bad_pivot(double d) { return !(d > 0.0); }

// In-place Cholesky factor of the 64 x 64 block in a[DC_NB][DC_LD]; only the lower triangle is read and written.  Returns true when a pivot failed (every thread of the
// team returns the same value); the block then holds numbers nobody may use.  Team size: 1, or a multiple of 16.  The caller syncs before the call.
template <class Team>
PGO_DC_HD bool dc_factor_block(const Team& T, double* a) {
    bool bad = false;
    const int nx = T.size() < 16 ? 1 : 16, ny = T.size() < 16 ? 1 : T.size() / 16;
    const int tx = T.size() < 16 ? 0 : T.rank() % 16, ty = T.size() < 16 ? 0 : T.rank() / 16;
    for (int p = 0; p < DC_NB; ++p) {
        const double d = a[p * DC_LD + p];      // (stays in place until the last pass: nobody writes it during this step)
        bad = bad || dc_bad_pivot(d);
        const double s = sqrt(d);
        for (int i = p + 1 + T.rank(); i < DC_NB; i += T.size()) a[i * DC_LD + p] = a[i * DC_LD + p] / s;
        T.sync();
        for (int i = p + 1 + ty; i < DC_NB; i += ny) {
            const double lip = a[i * DC_LD + p];
            for (int j = p + 1 + tx; j <= i; j += nx) a[i * DC_LD + j] = a[i * DC_LD + j] - lip * a[j * DC_LD + p];
        }
        T.sync();
    }
    for (int p = T.rank(); p < DC_NB; p += T.size()) a[p * DC_LD + p] = sqrt(a[p * DC_LD + p]);
    T.sync();
    return bad;
}

// L y = v with the factored block in a; v[DC_NB] is used up, y[DC_NB] receives the solution (both shared by the team).  The caller syncs before the call.
template <class Team>
PGO_DC_HD void dc_forward_block(const Team& T, const double* a, double* v, double* y) {
    for (int p = 0; p < DC_NB; ++p) {
        const double yp = v[p] / a[p * DC_LD + p];
        if (T.rank() == 0) y[p] = yp;
        for (int i = p + 1 + T.rank(); i < DC_NB; i += T.size()) v[i] = v[i] - a[i * DC_LD + p] * yp;
        T.sync();
    }
}
// L^T x = v
template <class Team>
PGO_DC_HD void dc_backward_block(const Team& T, const double* a, double* v, double* x) {
    for (int p = DC_NB - 1; p >= 0; --p) {
        const double xp = v[p] / a[p * DC_LD + p];
        if (T.rank() == 0) x[p] = xp;
        for (int i = T.rank(); i < p; i += T.size()) v[i] = v[i] - a[p * DC_LD + i] * xp;
        T.sync();
    }
}

// the four partial sums of a 64-term product (terms 16 q .. 16 q + 15 each, ascending) in the order the sweeps add them
PGO_DC_HD double dc_sum4(double p0, double p1, double p2, double p3) { return (p0 + p1) + (p2 + p3); }

// the Gram products' column classes (dc_param_gram_block)
constexpr int DC_GRAM = 256;

// ---- the order of the block steps: what the launcher (one or two launches per call) and the host instantiation both run
template <class Ops>
inline void dc_factor_steps(int n, Ops& o) {
    const int nt = n / DC_NB;
    o.factor_first();                                   // the diagonal block of step 0
    for (int k = 0; k + 1 < nt; ++k) { o.panel(k); o.update(k); }      // update(k) leaves the diagonal block of step k + 1 factored
}
template <class Ops>
inline void dc_solve_steps(int n, Ops& o) {
    const int nt = n / DC_NB;
    for (int k = 0; k < nt; ++k) o.forward(k);
    for (int k = nt - 1; k >= 0; --k) o.backward(k);
}

// The forward substitution with many right-hand sides on the mt tile rows of W.  start_tile[R]: the block column of the first right-hand side of tile row R, ascending in R;
// in step k only the tile rows [0, rows) with start_tile <= k take part (skip = false: all of them, from step 0 — the same bits, tests/test_dense_cov_host.py).
template <class Ops>
inline void dc_cov_steps(int n, int mt, const int32_t* start_tile, bool skip, Ops& o) {
    const int nt = n / DC_NB;
    int rows = skip ? 0 : mt;
    for (int k = skip ? start_tile[0] : 0; k < nt; ++k) {
        while (rows < mt && start_tile[rows] <= k) ++rows;
        o.cov_solve(k, rows);
        if (k + 1 < nt) o.cov_update(k, rows);
    }
}

// ---- covariance blocks of pose AND switch parameters (pgo_covariance).  With H = [H_pp C; C^T diag(h)] over the keyframes' tangent entries and one entry per switch, and
// S = H_pp - C diag(h)^-1 C^T the Schur complement the factor is of, v_e = -c_e / h_e (twelve non-zeros: the rows of the edge's two keyframes) gives
//   Sigma_pp = S^-1,   Sigma_p,e = S^-1 v_e,   Sigma_e,f = delta_ef / h_e + v_e^T S^-1 v_f:
// w_e = L^-1 v_e is one more right-hand-side row of W beside the keyframes' unit rows, and every block is again a Gram product of rows of W.
// A "block id" below n_nodes is a node (rows 6 id .. 6 id + 5, six unit rows of W), n_nodes + s is switch s (one row of W).  sw_node[2 s], sw_node[2 s + 1]: the two
// nodes of switch s, or -1 for a side that has no row in the system (a constant keyframe); sw_c[12 s + 6 side + a]: its column of C; sw_h[s]: h.

// h of a requested switch must divide: positive and finite
PGO_DC_HD bool dc_bad_hss(double h) { return !(h > 0.0) || h > 1.7976931348623157e308; }

// One right-hand side into its zeroed row of W.  col >= 0: the column of a unit row's one; -1: a padding row; -2 - s: the row of switch s.  Returns true when the
// switch's h is unusable (nothing is written then).
PGO_DC_HD bool dc_param_rhs_row(double* wrow, int32_t col, const int32_t* sw_node, const double* sw_c, const double* sw_h) {
    if (col >= 0) { wrow[col] = 1.0; return false; }
    if (col == -1) return false;
    const size_t s = (size_t)(-2 - col);
    const double h = sw_h[s];
    if (dc_bad_hss(h)) return true;
    for (int side = 0; side < 2; ++side) {
        const int32_t node = sw_node[2 * s + side];
        if (node < 0) continue;
        for (int a = 0; a < 6; ++a) wrow[(size_t)node * 6 + a] = -sw_c[s * 12 + side * 6 + a] / h;
    }
    return false;
}

// One DA x DB block (DA, DB: 6 or 1), row-major in the leading DA DB entries of out[36], the rest 0: out[i * DB + j] = sum over the columns c0 <= c < n of
// wa[i * ld + c] * wb[j * ld + c] — column classes ascending, then the binary tree — over DA rows of wa and DB rows of wb (consecutive rows of W; c0 a multiple of DC_GRAM:
// the columns before it hold zeros in one of the two).  add: delta_ef / h_e of a switch paired with itself (else 0, not added).  part[6 * DC_GRAM] is shared by the team.
// Team size: 1, or a divisor of DC_GRAM.  The caller syncs before.
template <int DA, int DB, class Team>
PGO_DC_HD void dc_param_gram_block(const Team& T, const double* wa, const double* wb, size_t ld, int n, int c0, bool with_add, double add, double* part, double* out) {
    for (int i = 0; i < DA; ++i) {
        for (int cls = T.rank(); cls < DC_GRAM; cls += T.size()) {
            double acc[DB];
            for (int j = 0; j < DB; ++j) acc[j] = 0.0;
            for (int c = c0 + cls; c < n; c += DC_GRAM) {
                const double a = wa[(size_t)i * ld + c];
                for (int j = 0; j < DB; ++j) acc[j] = acc[j] + a * wb[(size_t)j * ld + c];
            }
            for (int j = 0; j < DB; ++j) part[j * DC_GRAM + cls] = acc[j];
        }
        T.sync();
        for (int s = DC_GRAM / 2; s >= 1; s >>= 1) {
            for (int e = T.rank(); e < DB * s; e += T.size()) { const int j = e / s, cls = e - j * s; part[j * DC_GRAM + cls] = part[j * DC_GRAM + cls] + part[j * DC_GRAM + cls + s]; }
            T.sync();
        }
        if (T.rank() == 0) for (int j = 0; j < DB; ++j) out[i * DB + j] = with_add ? add + part[j * DC_GRAM] : part[j * DC_GRAM];
        T.sync();
    }
    for (int e = DA * DB + T.rank(); e < 36; e += T.size()) out[e] = 0.0;
}
// ... chosen by the two sizes
template <class Team>
PGO_DC_HD void dc_param_gram(const Team& T, const double* wa, int da, const double* wb, int db, size_t ld, int n, int c0, bool with_add, double add, double* part, double* out) {
    if (da == 6 && db == 6) dc_param_gram_block<6, 6>(T, wa, wb, ld, n, c0, false, 0.0, part, out);
    else if (da == 6) dc_param_gram_block<6, 1>(T, wa, wb, ld, n, c0, false, 0.0, part, out);
    else if (db == 6) dc_param_gram_block<1, 6>(T, wa, wb, ld, n, c0, false, 0.0, part, out);
    else dc_param_gram_block<1, 1>(T, wa, wb, ld, n, c0, with_add, add, part, out);
}

// What the host prepares of a pgo_covariance request: the requested block ids deduplicated, six unit rows per node and one row per switch, ordered by the first non-zero
// column — the switch rows whose lower node is i, which start at column 6 i, then node i's own six rows, 6 i .. 6 i + 5; a switch without a node (both keyframes
// constant: an all-zero row, its variance is 1 / h alone) after everything — so that each tile row's first non-zero column ascends and dc_cov_steps' "started rows are a
// prefix" holds; padded to whole tile rows.  n: the order of the (padded) matrix.  sw_node is read for ids >= n_nodes only: a request of nodes alone may pass nullptr.
struct DcParamPlan {
    int m = 0, mt = 0;
    std::vector<int32_t> col;              // [m] as dc_param_rhs_row reads it
    std::vector<int32_t> first_col;        // [m] the first column the row may be non-zero in; n: none (an all-zero row)
    std::vector<int32_t> start_tile;       // [mt]; n / 64 for a tile row of all-zero rows: it never starts
    std::vector<int32_t> row_a, row_b;     // per pair: the first row of W of block a / block b
    std::vector<int32_t> dim_a, dim_b;     // ... and their sizes, 6 or 1
    std::vector<int32_t> self_switch;      // per pair: s when both ids are switch s, else -1
    DcParamPlan(int n, int32_t n_nodes, const int32_t* sw_node, int64_t n_pairs, const int32_t* ia, const int32_t* ib) {
        std::vector<int32_t> uniq(ia, ia + n_pairs);
        uniq.insert(uniq.end(), ib, ib + n_pairs);
        std::sort(uniq.begin(), uniq.end());
        uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
        struct Item { int32_t start, kind, u; };      // start: the node whose block column the rows begin in; kind 0 switch, 1 node; u: index into uniq
        const int32_t none = std::numeric_limits<int32_t>::max();
        std::vector<Item> items;
        size_t rows = 0;
        for (size_t u = 0; u < uniq.size(); ++u) {
            const int32_t id = uniq[u];
            if (id < n_nodes) { items.push_back(Item{id, 1, (int32_t)u}); rows += 6; continue; }
            const int32_t a = sw_node[2 * (size_t)(id - n_nodes)], b = sw_node[2 * (size_t)(id - n_nodes) + 1];
            const int32_t lo = a < 0 ? b : (b < 0 ? a : std::min(a, b));
            items.push_back(Item{lo < 0 ? none : lo, 0, (int32_t)u}); rows += 1;
        }
        std::sort(items.begin(), items.end(), [](const Item& x, const Item& y) { return x.start != y.start ? x.start < y.start : (x.kind != y.kind ? x.kind < y.kind : x.u < y.u); });
        m = (int)((rows + DC_NB - 1) / DC_NB * DC_NB); mt = m / DC_NB;
        col.assign((size_t)m, -1); first_col.assign((size_t)m, n);
        std::vector<int32_t> row_of(uniq.size(), 0);
        int32_t r = 0;
        for (const Item& it : items) {
            row_of[(size_t)it.u] = r;
            const int32_t id = uniq[(size_t)it.u];
            if (it.kind == 1) { for (int a = 0; a < 6; ++a, ++r) col[(size_t)r] = first_col[(size_t)r] = id * 6 + a; }
            else { col[(size_t)r] = -2 - (id - n_nodes); first_col[(size_t)r] = it.start == none ? n : it.start * 6; ++r; }
        }
        for (int R = 0; R < mt; ++R) start_tile.push_back(first_col[(size_t)R * DC_NB] / DC_NB);
        auto at = [&](int32_t id) { return (size_t)(std::lower_bound(uniq.begin(), uniq.end(), id) - uniq.begin()); };
        for (int64_t k = 0; k < n_pairs; ++k) {
            row_a.push_back(row_of[at(ia[k])]); row_b.push_back(row_of[at(ib[k])]);
            dim_a.push_back(ia[k] < n_nodes ? 6 : 1); dim_b.push_back(ib[k] < n_nodes ? 6 : 1);
            self_switch.push_back(ia[k] >= n_nodes && ia[k] == ib[k] ? ia[k] - n_nodes : -1);
        }
    }
    // the first column in which both blocks' right-hand sides may be non-zero, rounded down to the Gram's column classes (a node's rows: that of its first row)
    int gram_c0(int64_t pair) const { return std::max(first_col[(size_t)row_a[(size_t)pair]], first_col[(size_t)row_b[(size_t)pair]]) / DC_GRAM * DC_GRAM; }
};

// ---- the matrix on a handle that keeps no block-CSR values (PGO_LINEAR_PCG_MATRIX_FREE): S assembled from the normal blocks of the last linearisation — Hd [N][36],
// J1^T J2 per edge (rows of c1, columns of c2), the switch couplings c [Es][12] and h [Es].  The host plan, built per call from the edge lists: the relative-pose and
// switchable edges with two distinct free keyframes sorted by (higher keyframe, lower keyframe), then by internal edge index (relative-pose before switchable) — one
// segment per keyframe pair = one lower-triangle off-diagonal block, written once as the sum over the segment in list order; and per keyframe its switchable edge sides
// in edge order, whose Schur terms come off the diagonal block.
struct DcMfPlan {
    std::vector<int32_t> seg_ptr, seg_hi, seg_lo;      // [segments + 1], [segments], [segments]
    std::vector<int32_t> ent;                          // per segment entry: index inside its class << 2 | switchable << 1 | transposed (the edge's c1 is the LOWER keyframe)
    std::vector<int32_t> side_ptr, side;               // [N + 1]; switchable edge << 1 | side
    DcMfPlan(int64_t N, const uint8_t* node_free, int64_t n_rel, const int32_t* rc1, const int32_t* rc2, int64_t n_sw, const int32_t* sc1, const int32_t* sc2) {
        struct E { int32_t hi, lo, order, ent; };
        std::vector<E> es;
        for (int cls = 0; cls < 2; ++cls) {
            const int64_t ne = cls ? n_sw : n_rel;
            const int32_t* c1 = cls ? sc1 : rc1; const int32_t* c2 = cls ? sc2 : rc2;
            for (int64_t e = 0; e < ne; ++e) {
                const int32_t a = c1[e], b = c2[e];
                if (a == b || a < 0 || b < 0 || a >= N || b >= N || !node_free[a] || !node_free[b]) continue;
                es.push_back(E{std::max(a, b), std::min(a, b), (int32_t)(cls ? n_rel + e : e), (int32_t)((e << 2) | (cls << 1) | (a < b ? 1 : 0))});
            }
        }
        std::sort(es.begin(), es.end(), [](const E& x, const E& y) { return x.hi != y.hi ? x.hi < y.hi : (x.lo != y.lo ? x.lo < y.lo : x.order < y.order); });
        for (size_t k = 0; k < es.size(); ++k) {
            if (k == 0 || es[k].hi != es[k - 1].hi || es[k].lo != es[k - 1].lo) { seg_ptr.push_back((int32_t)k); seg_hi.push_back(es[k].hi); seg_lo.push_back(es[k].lo); }
            ent.push_back(es[k].ent);
        }
        seg_ptr.push_back((int32_t)es.size());
        side_ptr.assign((size_t)N + 1, 0);
        for (int64_t e = 0; e < n_sw; ++e) for (int32_t nd : {sc1[e], sc2[e]}) if (nd >= 0 && nd < N) ++side_ptr[(size_t)nd + 1];
        for (int64_t i = 0; i < N; ++i) side_ptr[(size_t)i + 1] += side_ptr[(size_t)i];
        side.assign((size_t)side_ptr[(size_t)N], 0);
        std::vector<int32_t> fill(side_ptr.begin(), side_ptr.end() - 1);
        for (int64_t e = 0; e < n_sw; ++e) for (int s = 0; s < 2; ++s) { const int32_t nd = s ? sc2[e] : sc1[e]; if (nd >= 0 && nd < N) side[(size_t)fill[(size_t)nd]++] = (int32_t)((e << 1) | s); }
    }
    int64_t segments() const { return (int64_t)seg_hi.size(); }
};
// entry (a, c) of the off-diagonal block of one segment [b, e) of DcMfPlan::ent: rows of the higher keyframe, columns of the lower
PGO_DC_HD double dc_mf_offdiag_entry(const int32_t* ent, int32_t b, int32_t e, int a, int c, const double* hoff_rel, const double* hoff_sw, const double* sw_c, const double* sw_h) {
    double acc = 0.0;
    for (int32_t k = b; k < e; ++k) {
        const int32_t w = ent[k];
        const bool tr = (w & 1) != 0, sw = (w & 2) != 0;
        const size_t idx = (size_t)(w >> 2);
        const double* H = (sw ? hoff_sw : hoff_rel) + idx * 36;
        double v = tr ? H[c * 6 + a] : H[a * 6 + c];
        if (sw) {
            const double* cc = sw_c + idx * 12;
            const double cross = cc[(tr ? 6 : 0) + a] * cc[(tr ? 0 : 6) + c];
            v = v - cross / sw_h[idx];
        }
        acc = acc + v;
    }
    return acc;
}
// entry (a, c) of a free keyframe's diagonal block: hd (its 36 of Hd) minus the Schur terms of its switchable edge sides [b, e) of DcMfPlan::side
PGO_DC_HD double dc_mf_diag_entry(const double* hd, const int32_t* side, int32_t b, int32_t e, int a, int c, const double* sw_c, const double* sw_h) {
    double acc = hd[a * 6 + c];
    for (int32_t k = b; k < e; ++k) {
        const int32_t w = side[k];
        const double* cc = sw_c + (size_t)(w >> 1) * 12 + (w & 1) * 6;
        const double sq = cc[a] * cc[c];
        acc = acc - sq / sw_h[(size_t)(w >> 1)];
    }
    return acc;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- serial host instantiation: the same block steps, the same block routines, scalar loops where the kernels use the fp64 MFMA (sums over k ascending, formed from zero
// and then subtracted, as the accumulators are)
struct DcHost {
    int n; double* A; double* w; double* yv; double* x; bool failed = false;
    std::vector<double> blk = std::vector<double>((size_t)DC_NB * DC_LD, 0.0);
    double vec[DC_NB], sol[DC_NB];
    void load_block(int k0) { for (int i = 0; i < DC_NB; ++i) for (int j = 0; j < DC_NB; ++j) blk[(size_t)i * DC_LD + j] = A[(size_t)(k0 + i) * n + k0 + j]; }
    void factor_block(int k0) {
        load_block(k0);
        failed = dc_factor_block(DcSerial{}, blk.data()) || failed;
        for (int i = 0; i < DC_NB; ++i) for (int j = 0; j <= i; ++j) A[(size_t)(k0 + i) * n + k0 + j] = blk[(size_t)i * DC_LD + j];
    }
    void factor_first() { factor_block(0); }
    // one row of the panel's substitution: row[0 .. 63] <- row L_kk^-T, by 16-wide sub-blocks (what one lane column of dc_panel_kernel computes)
    static void substitute_row(const double* l, double* row) {
        for (int j = 0; j < DC_NB / DC_SUB; ++j) {
            double rr[DC_SUB];
            for (int c = 0; c < DC_SUB; ++c) {
                double acc = 0.0;
                for (int kk = 0; kk < j * DC_SUB; ++kk) acc += l[(size_t)(j * DC_SUB + c) * DC_LD + kk] * row[kk];
                rr[c] = row[j * DC_SUB + c] - acc;
            }
            for (int p = 0; p < DC_SUB; ++p) {
                const double yp = rr[p] / l[(size_t)(j * DC_SUB + p) * DC_LD + j * DC_SUB + p];
                rr[p] = yp;
                for (int q = p + 1; q < DC_SUB; ++q) rr[q] = rr[q] - l[(size_t)(j * DC_SUB + q) * DC_LD + j * DC_SUB + p] * yp;
            }
            for (int c = 0; c < DC_SUB; ++c) row[j * DC_SUB + c] = rr[c];
        }
    }
    void panel(int k) {
        const int k0 = k * DC_NB;
        load_block(k0);
        for (int r = k0 + DC_NB; r < n; ++r) substitute_row(blk.data(), A + (size_t)r * n + k0);
    }
    void update(int k) {
        const int k0 = k * DC_NB, k1 = k0 + DC_NB;
        for (int i = k1; i < n; ++i)
            for (int j = k1; j <= i; ++j) {
                double acc = 0.0;
                for (int kk = 0; kk < DC_NB; ++kk) acc += A[(size_t)i * n + k0 + kk] * A[(size_t)j * n + k0 + kk];
                A[(size_t)i * n + j] -= acc;
            }
        factor_block(k1);
    }
    void forward(int k) {
        const int k0 = k * DC_NB;
        load_block(k0);
        for (int i = 0; i < DC_NB; ++i) vec[i] = w[k0 + i];
        dc_forward_block(DcSerial{}, blk.data(), vec, sol);
        for (int i = 0; i < DC_NB; ++i) yv[k0 + i] = sol[i];
        for (int r = k0 + DC_NB; r < n; ++r) {
            double part[4];
            for (int q = 0; q < 4; ++q) { double s = 0.0; for (int c = 16 * q; c < 16 * q + 16; ++c) s += A[(size_t)r * n + k0 + c] * sol[c]; part[q] = s; }
            w[r] -= dc_sum4(part[0], part[1], part[2], part[3]);
        }
    }
    void backward(int k) {
        const int k0 = k * DC_NB;
        load_block(k0);
        for (int i = 0; i < DC_NB; ++i) vec[i] = yv[k0 + i];
        dc_backward_block(DcSerial{}, blk.data(), vec, sol);
        for (int i = 0; i < DC_NB; ++i) x[k0 + i] = sol[i];
        for (int c = 0; c < k0; ++c) {
            double part[4];
            for (int q = 0; q < 4; ++q) { double s = 0.0; for (int r = 16 * q; r < 16 * q + 16; ++r) s += A[(size_t)(k0 + r) * n + c] * sol[r]; part[q] = s; }
            yv[c] -= dc_sum4(part[0], part[1], part[2], part[3]);
        }
    }
    // covariance: the right-hand sides W[m][n] on the factor in A
    double* W = nullptr;
    void cov_solve(int k, int rows) {
        const int k0 = k * DC_NB;
        load_block(k0);
        for (int r = 0; r < rows * DC_NB; ++r) substitute_row(blk.data(), W + (size_t)r * n + k0);
    }
    void cov_update(int k, int rows) {
        const int k0 = k * DC_NB;
        for (int r = 0; r < rows * DC_NB; ++r)
            for (int c = k0 + DC_NB; c < n; ++c) {
                double acc = 0.0;
                for (int kk = 0; kk < DC_NB; ++kk) acc += W[(size_t)r * n + k0 + kk] * A[(size_t)c * n + k0 + kk];
                W[(size_t)r * n + c] -= acc;
            }
    }
};

// pgo_covariance's blocks on the host: `a` is S (n x n, padded like dc_host_solve; node i = rows 6 i .. 6 i + 5, n / 6 nodes), the n_sw switches as DcParamPlan takes
// them; block ids ia, ib in [0, n / 6 + n_sw).  cov: n_pairs x 36.  Returns false — and leaves cov alone — when a pivot failed or a requested switch's h is unusable.
inline bool dc_host_param_covariance(int n, const double* a, const int32_t* sw_node, const double* sw_c, const double* sw_h, int64_t n_pairs, const int32_t* ia, const int32_t* ib, bool skip, double* cov) {
    const int nc = (n + DC_NB - 1) / DC_NB * DC_NB;
    std::vector<double> A((size_t)nc * nc, 0.0);
    for (int i = 0; i < nc; ++i) {
        if (i < n) { for (int j = 0; j < n; ++j) A[(size_t)i * nc + j] = a[(size_t)i * n + j]; }
        else A[(size_t)i * nc + i] = 1.0;
    }
    DcHost H{nc, A.data(), nullptr, nullptr, nullptr};
    dc_factor_steps(nc, H);
    if (H.failed) return false;
    const DcParamPlan Q(nc, n / 6, sw_node, n_pairs, ia, ib);
    std::vector<double> W((size_t)Q.m * nc, 0.0), part((size_t)6 * DC_GRAM), blocks((size_t)36 * n_pairs);
    for (int r = 0; r < Q.m; ++r) if (dc_param_rhs_row(W.data() + (size_t)r * nc, Q.col[(size_t)r], sw_node, sw_c, sw_h)) return false;
    H.W = W.data();
    dc_cov_steps(nc, Q.mt, Q.start_tile.data(), skip, H);      // (nothing but all-zero rows: start_tile[0] = nc / 64, no step runs)
    for (int64_t k = 0; k < n_pairs; ++k) {
        const int32_t s = Q.self_switch[(size_t)k];
        dc_param_gram(DcSerial{}, W.data() + (size_t)Q.row_a[(size_t)k] * nc, Q.dim_a[(size_t)k], W.data() + (size_t)Q.row_b[(size_t)k] * nc, Q.dim_b[(size_t)k], (size_t)nc, nc,
                      skip ? Q.gram_c0(k) : 0, s >= 0, s >= 0 ? 1.0 / sw_h[(size_t)s] : 0.0, part.data(), blocks.data() + 36 * k);
    }
    std::copy(blocks.begin(), blocks.end(), cov);
    return true;
}

// The matrix DcMfPlan describes, on the host: the lower triangle (and the whole diagonal blocks) of the zeroed n x n `A`, n >= 6 N a multiple of 64; identity rows for
// keyframes that are not free and for the padding.  hoff: the relative-pose edges' blocks, then the switchable edges' (36 each, contiguous).
inline void dc_host_mf_matrix(int64_t N, const uint8_t* node_free, int64_t n_rel, const DcMfPlan& M, const double* hd, const double* hoff, const double* sw_c, const double* sw_h, int n, double* A) {
    for (int64_t i = 0; i < N; ++i)
        for (int a = 0; a < 6; ++a)
            for (int c = 0; c < 6; ++c) {
                const size_t row = (size_t)i * 6 + a, colm = (size_t)i * 6 + c;
                if (node_free[i]) A[row * n + colm] = dc_mf_diag_entry(hd + (size_t)i * 36, M.side.data(), M.side_ptr[(size_t)i], M.side_ptr[(size_t)i + 1], a, c, sw_c, sw_h);
                else if (a == c) A[row * n + colm] = 1.0;
            }
    for (size_t i = (size_t)N * 6; i < (size_t)n; ++i) A[i * n + i] = 1.0;
    for (int64_t s = 0; s < M.segments(); ++s)
        for (int a = 0; a < 6; ++a)
            for (int c = 0; c < 6; ++c)
                A[((size_t)M.seg_hi[(size_t)s] * 6 + a) * n + (size_t)M.seg_lo[(size_t)s] * 6 + c] =
                    dc_mf_offdiag_entry(M.ent.data(), M.seg_ptr[(size_t)s], M.seg_ptr[(size_t)s + 1], a, c, hoff, hoff + (size_t)n_rel * 36, sw_c, sw_h);
}

// Solves A x = b for the symmetric positive definite n x n matrix `a` (row-major, any n >= 1: padded to a multiple of 64 by an identity block).  Returns false — and leaves
// x alone — when a pivot failed.
inline bool dc_host_solve(int n, const double* a, const double* b, double* x) {
    const int nc = (n + DC_NB - 1) / DC_NB * DC_NB;
    std::vector<double> A((size_t)nc * nc, 0.0), w((size_t)nc, 0.0), yv((size_t)nc, 0.0), xs((size_t)nc, 0.0);
    for (int i = 0; i < nc; ++i) {
        if (i < n) { for (int j = 0; j < n; ++j) A[(size_t)i * nc + j] = a[(size_t)i * n + j]; w[i] = b[i]; }
        else A[(size_t)i * nc + i] = 1.0;
    }
    DcHost H{nc, A.data(), w.data(), yv.data(), xs.data()};
    dc_factor_steps(nc, H);
    if (H.failed) return false;
    dc_solve_steps(nc, H);
    for (int i = 0; i < n; ++i) x[i] = xs[i];
    return true;
}
#endif

}  // namespace pgo
