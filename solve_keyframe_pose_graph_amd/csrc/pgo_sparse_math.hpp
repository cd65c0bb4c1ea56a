// pgo_sparse_math.hpp — the host side of a tile-sparse exact Cholesky solver for graphs above the dense solver's limit (pgo_dense.hip stops at PGO_DENSE_MAX_KEYFRAMES
// because it stores all n^2 entries): the ordering of the keyframes, the tile pattern of the system, the symbolic factorisation, the order of the block steps and a serial
// host instantiation of the whole factor and solve (tests/native/sparse_chol_host.cpp), of the selected inverse on the factor's tiles (sc_selinv_steps, ScSelHost;
// tests/native/sparse_selinv_host.cpp) and of both sweeps over panels of 64 right-hand sides (sc_panel_steps, ScPanelHost; tests/native/sparse_panel_host.cpp).  The arithmetic is pgo_dense_math.hpp's: the same 64 x 64 block routines, the same
// panel substitution, the same update.  libpgo.so does not include this header and no option of pgo_options uses it (DESIGN.md section 3.4 says why); the kernels that run
// this plan and this step order are the companion library's, libpgo_sparse.so (pgo_sparse.hip, include/pgo_sparse.h).
//
// The matrix is the dense solver's — n = 6 N padded to a multiple of 64, identity on the padding and on the rows of keyframes outside the system — with its rows and
// columns in a permuted order of the keyframes, and only the 64 x 64 tiles of the lower triangle that the factor L can be non-zero in are stored: `tiles` x 4096 doubles,
// each tile row-major, tile ids in row order (the tiles of tile row i by ascending column, the diagonal tile last).  A tile-level symbolic Cholesky gives them: with s_k the
// tile rows below the diagonal of column k of L,  s_k = (tile rows of A in column k) U (s_c \ {k} for every column c whose first entry min s_c is k)  — the elimination
// tree, a column's structure merged into its parent's.
//
// Per block step k (sc_factor_steps) the dense algorithm's two steps run on s_k alone:
//   panel   L_ik = A_ik L_kk^-T for i in s_k;
//   update  A_ij -= L_ik L_jk^T for every pair i >= j of s_k — tile (i, j) is in the pattern by construction — and the diagonal tile k + 1 is factored by the update
//           when k + 1 is in s_k, by a step of its own otherwise (an empty s_k runs neither panel nor update).
// Every tile operation of the dense algorithm that is skipped here would have produced or subtracted a zero: an accumulator that starts at +0 and only ever adds
// products with a zero factor stays +0, and old - (+0) = old.  In the trajectory's natural order the factor and the solution are therefore the dense solver's AS NUMBERS
// (tests/test_sparse_cholesky_host.py holds sc_host_solve to dc_host_solve that way); under another order they are another rounding of the same exact solution.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <numeric>
#include <utility>
#include <vector>

#include "pgo_dense_math.hpp"

namespace pgo {

constexpr size_t SC_TILE = (size_t)DC_NB * DC_NB;      // doubles of one stored tile

// ---- ordering: a permutation of the keyframes.  order[q] = the keyframe at position q.
// adj_ptr / adj: per keyframe its neighbours (any order, duplicates and the keyframe itself allowed); in_system[i] = 0: a constant or unreferenced keyframe.
inline std::vector<int32_t> sc_order_natural(int64_t N) {
    std::vector<int32_t> order((size_t)N);
    std::iota(order.begin(), order.end(), 0);
    return order;
}
// Reverse Cuthill-McKee on the keyframes of the system; deterministic: every component starts at its keyframe of lowest (degree, index) among those not yet numbered,
// neighbours are taken by (degree, index), the whole numbering is reversed; the keyframes outside the system follow, by index.
inline std::vector<int32_t> sc_order_rcm(int64_t N, const int64_t* adj_ptr, const int32_t* adj, const uint8_t* in_system) {
    std::vector<std::vector<int32_t>> nb((size_t)N);
    for (int64_t i = 0; i < N; ++i) {
        if (!in_system[i]) continue;
        std::vector<int32_t>& v = nb[(size_t)i];
        for (int64_t b = adj_ptr[i]; b < adj_ptr[i + 1]; ++b) { const int32_t j = adj[b]; if (j != i && j >= 0 && j < N && in_system[j]) v.push_back(j); }
        std::sort(v.begin(), v.end());
        v.erase(std::unique(v.begin(), v.end()), v.end());
    }
    auto before = [&](int32_t a, int32_t b) { return nb[(size_t)a].size() != nb[(size_t)b].size() ? nb[(size_t)a].size() < nb[(size_t)b].size() : a < b; };
    std::vector<int32_t> starts;
    for (int64_t i = 0; i < N; ++i) if (in_system[i]) starts.push_back((int32_t)i);
    std::sort(starts.begin(), starts.end(), before);
    std::vector<uint8_t> seen((size_t)N, 0);
    std::vector<int32_t> cm;
    cm.reserve((size_t)N);
    for (int32_t s : starts) {
        if (seen[(size_t)s]) continue;
        seen[(size_t)s] = 1;
        size_t head = cm.size();
        cm.push_back(s);
        while (head < cm.size()) {
            const int32_t u = cm[head++];
            const size_t first = cm.size();
            for (int32_t v : nb[(size_t)u]) if (!seen[(size_t)v]) { seen[(size_t)v] = 1; cm.push_back(v); }
            std::sort(cm.begin() + (std::ptrdiff_t)first, cm.end(), before);
        }
    }
    std::reverse(cm.begin(), cm.end());
    for (int64_t i = 0; i < N; ++i) if (!in_system[i]) cm.push_back((int32_t)i);
    return cm;
}

// ---- the plan: tile pattern of L by row and by column, tile ids, counts
struct ScPlan {
    int nt = 0;
    std::vector<int32_t> row_ptr, row_col;                 // [nt + 1], [tiles]: the tiles of tile row i, columns ascending, the diagonal last; the index into row_col IS the tile id
    std::vector<int32_t> col_ptr, col_row, col_tile;       // [nt + 1], then per column k the sorted rows of s_k and the ids of the tiles (row, k)
    std::vector<uint8_t> ahead;                            // [nt]: k + 1 is in s_k — the update of step k factors the diagonal tile k + 1
    int64_t a_tiles = 0;                                   // non-zero lower tiles of the matrix (diagonal included)
    int64_t tiles() const { return (int64_t)row_col.size(); }
    int s_size(int k) const { return col_ptr[(size_t)k + 1] - col_ptr[(size_t)k]; }
    int diag(int k) const { return row_ptr[(size_t)k + 1] - 1; }
    int max_s() const { int m = 0; for (int k = 0; k < nt; ++k) m = std::max(m, s_size(k)); return m; }
    // the id of tile (i, j), j <= i; -1: not in the pattern
    int find(int i, int j) const {
        const auto b = row_col.begin() + row_ptr[(size_t)i], e = row_col.begin() + row_ptr[(size_t)i + 1];
        const auto it = std::lower_bound(b, e, (int32_t)j);
        return it != e && *it == j ? (int)(it - row_col.begin()) : -1;
    }
    int64_t factor_launches() const { int64_t l = 1; for (int k = 0; k + 1 < nt; ++k) l += s_size(k) > 0 ? (ahead[(size_t)k] ? 2 : 3) : 1; return l; }
    int64_t solve_launches() const { return 2 * (int64_t)nt; }
    int64_t tile_updates() const { int64_t u = 0; for (int k = 0; k < nt; ++k) { const int64_t m = s_size(k); u += m * (m + 1) / 2; } return u; }
    // the selected inverse (sc_selinv_steps): one launch for the inverses of all diagonal tiles, then ginv + column + diag per column with a non-empty s_k; tile products:
    // |s_k|^2 of column(k) and |s_k| of diag(k)
    int64_t selinv_launches() const { int64_t l = 1; for (int k = 0; k < nt; ++k) l += s_size(k) > 0 ? 3 : 0; return l; }
    int64_t selinv_products() const { int64_t u = 0; for (int k = 0; k < nt; ++k) { const int64_t m = s_size(k); u += m * m + m; } return u; }
    // the panel sweeps (sc_panel_steps) of n_panels panels with first[] ascending and the lowest requested tile k_stop: one launch per step of the two sweeps; tile
    // products: forward, per step k and started panel p the stored tiles (k, j) with first[p] <= j < k; backward, |s_k| per step k >= k_stop and panel
    int64_t panel_launches(const int32_t* first, int n_panels, int k_stop) const { return n_panels > 0 ? (int64_t)(nt - first[0]) + (nt - k_stop) : 0; }
    int64_t panel_products(const int32_t* first, int n_panels, int k_stop) const {
        int64_t u = 0;
        for (int p = 0; p < n_panels; ++p)
            for (int k = first[p]; k < nt; ++k)
                u += (row_col.begin() + diag(k)) - std::lower_bound(row_col.begin() + row_ptr[(size_t)k], row_col.begin() + diag(k), first[p]);
        for (int k = k_stop; k < nt; ++k) u += (int64_t)n_panels * s_size(k);
        return u;
    }
    size_t scratch_doubles() const { return (size_t)DC_NB * ((size_t)max_s() * DC_NB + 16); }      // the k-major copy of one panel, compact by position in s_k (>= max_s tiles: the selected inverse keeps G there)
    int ldu() const { return max_s() * DC_NB + 16; }
};

// Symbolic factorisation.  below[j]: the tile rows i > j of the matrix's non-zero lower tiles in column j (any order, duplicates allowed); every diagonal tile is present.
inline ScPlan sc_symbolic(int nt, std::vector<std::vector<int32_t>> below) {
    ScPlan P;
    P.nt = nt;
    P.a_tiles = nt;
    for (int k = 0; k < nt; ++k) {
        std::vector<int32_t>& s = below[(size_t)k];
        std::sort(s.begin(), s.end());
        s.erase(std::unique(s.begin(), s.end()), s.end());
        P.a_tiles += (int64_t)s.size();
    }
    for (int k = 0; k < nt; ++k) {      // (children come before their parent: by the time column k is read, every structure that merges into it has)
        std::vector<int32_t>& s = below[(size_t)k];
        std::sort(s.begin(), s.end());
        s.erase(std::unique(s.begin(), s.end()), s.end());
        if (s.size() > 1) { std::vector<int32_t>& parent = below[(size_t)s[0]]; parent.insert(parent.end(), s.begin() + 1, s.end()); }
    }
    std::vector<int32_t> count((size_t)nt, 1);      // tiles of every row: the diagonal ...
    for (int k = 0; k < nt; ++k) for (int32_t i : below[(size_t)k]) ++count[(size_t)i];
    P.row_ptr.assign((size_t)nt + 1, 0);
    for (int i = 0; i < nt; ++i) P.row_ptr[(size_t)i + 1] = P.row_ptr[(size_t)i] + count[(size_t)i];
    P.row_col.assign((size_t)P.row_ptr[(size_t)nt], 0);
    std::vector<int32_t> fill(P.row_ptr.begin(), P.row_ptr.end() - 1);
    P.col_ptr.assign((size_t)nt + 1, 0);
    P.ahead.assign((size_t)nt, 0);
    for (int k = 0; k < nt; ++k) {      // (columns ascending: every row's list comes out sorted)
        const std::vector<int32_t>& s = below[(size_t)k];
        P.col_ptr[(size_t)k + 1] = P.col_ptr[(size_t)k] + (int32_t)s.size();
        P.ahead[(size_t)k] = !s.empty() && s[0] == k + 1;
        for (int32_t i : s) { P.col_row.push_back(i); P.col_tile.push_back(fill[(size_t)i]); P.row_col[(size_t)fill[(size_t)i]++] = k; }
    }
    for (int i = 0; i < nt; ++i) P.row_col[(size_t)fill[(size_t)i]] = i;
    return P;
}

// The tile pattern of a pose graph's system under an order of its keyframes: the diagonal block of every keyframe and one block per pair of neighbours, six rows per
// keyframe at 6 pos[keyframe] — which may straddle two tile rows and two tile columns: every scalar entry on or below the diagonal marks its tile.
inline std::vector<std::vector<int32_t>> sc_graph_pattern(int64_t N, const int64_t* adj_ptr, const int32_t* adj, const uint8_t* in_system, const int32_t* pos, int nt) {
    std::vector<std::vector<int32_t>> below((size_t)nt);
    for (int64_t i = 0; i < N; ++i) {
        if (!in_system[i]) continue;
        const int64_t r0 = (int64_t)pos[i] * 6;
        for (int64_t b = adj_ptr[i]; b <= adj_ptr[i + 1]; ++b) {      // (the last round: the keyframe's own diagonal block)
            const int32_t j = b < adj_ptr[i + 1] ? adj[b] : (int32_t)i;
            if (j < 0 || j >= N || !in_system[j] || pos[j] > pos[i]) continue;
            const int64_t c0 = (int64_t)pos[j] * 6;
            const int ti0 = (int)(r0 / DC_NB), ti1 = (int)((r0 + 5) / DC_NB), tj0 = (int)(c0 / DC_NB), tj1 = (int)((c0 + 5) / DC_NB);
            for (int ti = ti0; ti <= ti1; ++ti)
                for (int tj = tj0; tj <= tj1; ++tj) {
                    if (tj >= ti) continue;      // the diagonal tiles are always there
                    // (rows of tile ti inside the block x columns of tile tj inside the block: never empty, and every such entry lies below the diagonal)
                    std::vector<int32_t>& v = below[(size_t)tj];
                    if (v.empty() || v.back() != ti) v.push_back(ti);
                }
        }
    }
    return below;
}

// Ordering + plan of a graph.  ordering: -1 both orders, the one with fewer tiles of L (natural on a tie); 0 natural; 1 reverse Cuthill-McKee.  *used: 0 or 1.
inline ScPlan sc_plan_graph(int64_t N, const int64_t* adj_ptr, const int32_t* adj, const uint8_t* in_system, int ordering, std::vector<int32_t>& order, int* used) {
    const int n = std::max<int>(DC_NB, (int)((N * 6 + DC_NB - 1) / DC_NB * DC_NB)), nt = n / DC_NB;
    auto plan_of = [&](const std::vector<int32_t>& ord) {
        std::vector<int32_t> pos((size_t)N);
        for (int64_t q = 0; q < N; ++q) pos[(size_t)ord[(size_t)q]] = (int32_t)q;
        return sc_symbolic(nt, sc_graph_pattern(N, adj_ptr, adj, in_system, pos.data(), nt));
    };
    ScPlan natural, rcm;
    std::vector<int32_t> o_rcm;
    if (ordering != 1) natural = plan_of(sc_order_natural(N));
    if (ordering != 0) { o_rcm = sc_order_rcm(N, adj_ptr, adj, in_system); rcm = plan_of(o_rcm); }
    const bool take_rcm = ordering == 1 || (ordering != 0 && rcm.tiles() < natural.tiles());
    *used = take_rcm ? 1 : 0;
    order = take_rcm ? o_rcm : sc_order_natural(N);
    return take_rcm ? rcm : natural;
}

// ---- the order of the block steps: what the host instantiation runs, and what a launcher of kernels would
template <class Ops>
inline void sc_factor_steps(const ScPlan& P, Ops& o) {
    o.factor_diag(0, true);                              // the diagonal tile of step 0 (first = true: the step a forced failure would be raised in)
    for (int k = 0; k + 1 < P.nt; ++k) {
        const bool any = P.s_size(k) > 0;
        if (any) { o.panel(k); o.update(k); }            // update(k) leaves the diagonal tile k + 1 factored when k + 1 is in s_k
        if (!any || !P.ahead[(size_t)k]) o.factor_diag(k + 1, false);
    }
}
template <class Ops>
inline void sc_solve_steps(const ScPlan& P, Ops& o) {
    for (int k = 0; k < P.nt; ++k) o.forward(k);
    for (int k = P.nt - 1; k >= 0; --k) o.backward(k);
}
// The selected inverse (Takahashi's recurrence on the tiles of L): every tile of Z = A^-1 that lies in the pattern of L, one backward pass over the block columns.
// With A = L L^T and s = s_k:
//   inverses() Z_kk = L_kk^-T L_kk^-1 for EVERY k, the entries i >= j, mirrored: it reads L alone, so it is one step of nt independent parts ahead of the chain of
//              dependent steps (on the device one launch of nt workgroups: the 64-step substitutions are the longest block routine of the recurrence);
// then for k = nt - 1 .. 0 with a non-empty s_k:
//   ginv(k)    G_e = L_{s[e],k} L_kk^-1 for every tile of s, by substitution, compact by position e;
//   column(k)  Z_{s[a],k} = - sum_b Z(s[a], s[b]) G_b, b ascending; Z(s[a], s[b]) = Z(s[b], s[a])^T where a < b — every tile (s[a], s[b]), a >= b, is in the pattern by
//              the argument the update relies on, and it was finished by the steps of the columns s[b] > k;
//   diag(k)    Z_kk -= sum_a G_a^T Z_{s[a],k}, the entries i >= j, mirrored: a diagonal tile of Z holds both triangles with equal bits.
// An empty s_k has no step: Z_kk = L_kk^-T L_kk^-1 alone.  Z is a second tile array with the ids of L's tiles; L is only read.
template <class Ops>
inline void sc_selinv_steps(const ScPlan& P, Ops& o) {
    o.inverses();
    for (int k = P.nt - 1; k >= 0; --k)
        if (P.s_size(k) > 0) { o.ginv(k); o.column(k); o.diag(k); }
}

// Columns of A^-1 in number — the blocks OUTSIDE the pattern of L, which the selected inverse has not: both sweeps with many right-hand sides at once.  The right-hand
// sides are the ROWS of W [m_pad][nc], m_pad a multiple of 64 (the dense covariance kernels' layout); a panel is 64 consecutive rows, W_pk the 64 x 64 block of panel p
// in the columns of tile k.  Row r starts as the unit row e_c^T; the forward sweep leaves y^T = e_c^T L^-T in it, the backward sweep x^T = y^T L^-1 = (A^-1 e_c)^T, in place.
// first[p]: the tile that holds the first non-zero of panel p; the rows are sorted by the column of their one, so first[] ascends and the panels that have started at
// step k are a prefix.  k_stop: the lowest tile that holds a requested entry of x — x_k needs x_i for i > k only, so the backward sweep ends there.
//   forward   k = first[0] .. nt - 1, every started panel p:   W_pk -= sum_j W_pj L_kj^T over the stored tiles (k, j), j < k, j ascending, j >= first[p];  W_pk <- W_pk L_kk^-T
//   backward  k = nt - 1 .. k_stop, every panel p:             W_pk -= sum_{i in s_k} W_pi L_ik, i ascending;                                              W_pk <- W_pk L_kk^-1
// The pull form: block W_pk has one writer, the step (k, p), which reads blocks of its own panel that earlier steps finished — no atomics, and one launch per k with a
// workgroup per panel.  Each sum is formed from zero in the order above and subtracted once; a product that is skipped (j < first[p], a panel that has not started) has
// an all-zero W_pj and would have added +0, and row r of a product reads row r of W alone: a right-hand side gets the same bits alone, in any batch and in any chunk,
// and whatever k_stop is.  pfwd(k, started) / pbwd(k, panels): one op per (k, panel), handed over per k.
template <class Ops>
inline void sc_panel_steps(const ScPlan& P, const std::vector<int32_t>& first, int k_stop, Ops& o) {
    const int np = (int)first.size();
    if (np == 0) return;
    int started = 0;
    for (int k = first[0]; k < P.nt; ++k) {
        while (started < np && first[(size_t)started] <= k) ++started;
        o.pfwd(k, started);
    }
    for (int k = P.nt - 1; k >= k_stop; --k) o.pbwd(k, np);
}

// The plan of a dense host matrix (n x n row-major, padded to nc = a multiple of 64 by identity rows): the tile pattern is that of the exact non-zeros of its lower
// triangle with row i at position pos[i] (pos = nullptr: where it is).
inline ScPlan sc_plan_matrix(int n, const double* a, const int32_t* pos) {
    const int nc = (n + DC_NB - 1) / DC_NB * DC_NB, nt = nc / DC_NB;
    std::vector<std::vector<int32_t>> below((size_t)nt);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            const int pi = pos ? pos[i] : i, pj = pos ? pos[j] : j;
            if (pj >= pi || a[(size_t)i * n + j] == 0.0) continue;
            if (pj / DC_NB < pi / DC_NB) below[(size_t)(pj / DC_NB)].push_back(pi / DC_NB);
        }
    return sc_symbolic(nt, std::move(below));
}
// ... and its tiles: the lower triangle (and the whole of the diagonal tiles' lower halves) of the permuted, padded matrix into zeroed tile storage
inline void sc_fill_tiles(const ScPlan& P, int n, const double* a, const int32_t* pos, double* T) {
    const int nc = P.nt * DC_NB;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            const int pi = pos ? pos[i] : i, pj = pos ? pos[j] : j;
            const double v = a[(size_t)i * n + j];
            if (pj > pi || v == 0.0) continue;
            T[(size_t)P.find(pi / DC_NB, pj / DC_NB) * SC_TILE + (size_t)(pi % DC_NB) * DC_NB + pj % DC_NB] = v;
        }
    for (int i = n; i < nc; ++i) T[(size_t)P.diag(i / DC_NB) * SC_TILE + (size_t)(i % DC_NB) * DC_NB + i % DC_NB] = 1.0;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- serial host instantiation on the tile storage: DcHost's arithmetic, tile by tile
struct ScHost {
    const ScPlan& P; double* T; double* w; double* yv; double* x; bool failed = false;
    std::vector<double> blk = std::vector<double>((size_t)DC_NB * DC_LD, 0.0);
    double vec[DC_NB], sol[DC_NB];
    double* tile(int id) const { return T + (size_t)id * SC_TILE; }
    void load_diag(int k) { const double* t = tile(P.diag(k)); for (int i = 0; i < DC_NB; ++i) for (int j = 0; j < DC_NB; ++j) blk[(size_t)i * DC_LD + j] = t[i * DC_NB + j]; }
    void factor_diag(int k, bool) {
        load_diag(k);
        failed = dc_factor_block(DcSerial{}, blk.data()) || failed;
        double* t = tile(P.diag(k));
        for (int i = 0; i < DC_NB; ++i) for (int j = 0; j <= i; ++j) t[i * DC_NB + j] = blk[(size_t)i * DC_LD + j];
    }
    void panel(int k) {
        load_diag(k);
        for (int32_t e = P.col_ptr[(size_t)k]; e < P.col_ptr[(size_t)k + 1]; ++e) {
            double* t = tile(P.col_tile[(size_t)e]);
            for (int r = 0; r < DC_NB; ++r) DcHost::substitute_row(blk.data(), t + (size_t)r * DC_NB);
        }
    }
    void update(int k) {
        const int32_t c0 = P.col_ptr[(size_t)k], m = P.s_size(k);
        for (int a = 0; a < m; ++a)
            for (int b = 0; b <= a; ++b) {
                const double* la = tile(P.col_tile[(size_t)(c0 + a)]); const double* lb = tile(P.col_tile[(size_t)(c0 + b)]);
                double* t = tile(P.find(P.col_row[(size_t)(c0 + a)], P.col_row[(size_t)(c0 + b)]));      // in the pattern by construction
                for (int i = 0; i < DC_NB; ++i)
                    for (int j = 0; j <= (a == b ? i : DC_NB - 1); ++j) {
                        double acc = 0.0;
                        for (int kk = 0; kk < DC_NB; ++kk) acc += la[i * DC_NB + kk] * lb[j * DC_NB + kk];
                        t[i * DC_NB + j] -= acc;
                    }
            }
        if (P.ahead[(size_t)k]) factor_diag(k + 1, false);
    }
    void forward(int k) {
        const int k0 = k * DC_NB;
        load_diag(k);
        for (int i = 0; i < DC_NB; ++i) vec[i] = w[k0 + i];
        dc_forward_block(DcSerial{}, blk.data(), vec, sol);
        for (int i = 0; i < DC_NB; ++i) yv[k0 + i] = sol[i];
        for (int32_t e = P.col_ptr[(size_t)k]; e < P.col_ptr[(size_t)k + 1]; ++e) {
            const double* t = tile(P.col_tile[(size_t)e]);
            const int i0 = P.col_row[(size_t)e] * DC_NB;
            for (int r = 0; r < DC_NB; ++r) {
                double part[4];
                for (int q = 0; q < 4; ++q) { double s = 0.0; for (int c = 16 * q; c < 16 * q + 16; ++c) s += t[r * DC_NB + c] * sol[c]; part[q] = s; }
                w[i0 + r] -= dc_sum4(part[0], part[1], part[2], part[3]);
            }
        }
    }
    void backward(int k) {
        const int k0 = k * DC_NB;
        load_diag(k);
        for (int i = 0; i < DC_NB; ++i) vec[i] = yv[k0 + i];
        dc_backward_block(DcSerial{}, blk.data(), vec, sol);
        for (int i = 0; i < DC_NB; ++i) x[k0 + i] = sol[i];
        for (int32_t id = P.row_ptr[(size_t)k]; id < P.diag(k); ++id) {
            const double* t = tile(id);
            const int j0 = P.row_col[(size_t)id] * DC_NB;
            for (int c = 0; c < DC_NB; ++c) {
                double part[4];
                for (int q = 0; q < 4; ++q) { double s = 0.0; for (int r = 16 * q; r < 16 * q + 16; ++r) s += t[r * DC_NB + c] * sol[r]; part[q] = s; }
                yv[j0 + c] -= dc_sum4(part[0], part[1], part[2], part[3]);
            }
        }
    }
};

// ---- serial host instantiation of the selected inverse on the factored tiles T: Z [tiles][4096] receives every tile, T is only read.  G and L_kk^-T L_kk^-1 come from
// the block substitutions (a row of G: L_kk^T g = l; a column of the inverse: L_kk y = e_c, L_kk^T x = y), never from a product with an explicit inverse; every product
// is a sum formed from zero in ascending order (b or a outermost, then the 64 terms) and subtracted once, as the kernels' accumulators are.
struct ScSelHost {
    const ScPlan& P; const double* T; double* Z;
    std::vector<double> G = std::vector<double>((size_t)std::max(P.max_s(), 1) * SC_TILE, 0.0);      // G_e row-major, compact by position in s_k
    std::vector<double> blk = std::vector<double>((size_t)DC_NB * DC_LD, 0.0), X = std::vector<double>((size_t)DC_NB * DC_LD, 0.0), acc = std::vector<double>(SC_TILE, 0.0);
    double vec[DC_NB], sol[DC_NB];
    double* ztile(int id) const { return Z + (size_t)id * SC_TILE; }
    void load_diag(int k) { const double* t = T + (size_t)P.diag(k) * SC_TILE; for (int i = 0; i < DC_NB; ++i) for (int j = 0; j < DC_NB; ++j) blk[(size_t)i * DC_LD + j] = t[i * DC_NB + j]; }
    void ginv(int k) {
        load_diag(k);
        const int32_t c0 = P.col_ptr[(size_t)k], m = P.s_size(k);
        for (int e = 0; e < m; ++e) {
            const double* t = T + (size_t)P.col_tile[(size_t)(c0 + e)] * SC_TILE;
            double* g = G.data() + (size_t)e * SC_TILE;
            for (int r = 0; r < DC_NB; ++r) {
                for (int c = 0; c < DC_NB; ++c) vec[c] = t[r * DC_NB + c];
                dc_backward_block(DcSerial{}, blk.data(), vec, sol);
                for (int c = 0; c < DC_NB; ++c) g[r * DC_NB + c] = sol[c];
            }
        }
    }
    void column(int k) {
        const int32_t c0 = P.col_ptr[(size_t)k], m = P.s_size(k);
        for (int a = 0; a < m; ++a) {
            std::fill(acc.begin(), acc.end(), 0.0);
            const int ra = P.col_row[(size_t)(c0 + a)];
            for (int b = 0; b < m; ++b) {
                const int rb = P.col_row[(size_t)(c0 + b)];
                const bool tr = a < b;                                           // the stored tile is (s[b], s[a]): read transposed
                const double* z = ztile(tr ? P.find(rb, ra) : P.find(ra, rb));      // in the pattern by construction
                const double* g = G.data() + (size_t)b * SC_TILE;
                for (int i = 0; i < DC_NB; ++i)
                    for (int n = 0; n < DC_NB; ++n) {
                        double s = acc[(size_t)i * DC_NB + n];
                        for (int kk = 0; kk < DC_NB; ++kk) s += (tr ? z[kk * DC_NB + i] : z[i * DC_NB + kk]) * g[kk * DC_NB + n];
                        acc[(size_t)i * DC_NB + n] = s;
                    }
            }
            double* out = ztile(P.col_tile[(size_t)(c0 + a)]);
            for (size_t e = 0; e < SC_TILE; ++e) out[e] = -acc[e];
        }
    }
    void inverses() {
        for (int k = 0; k < P.nt; ++k) {
            load_diag(k);
            for (int c = 0; c < DC_NB; ++c) {      // column c of L_kk^-T L_kk^-1 from the unit right-hand side e_c
                for (int i = 0; i < DC_NB; ++i) vec[i] = i == c ? 1.0 : 0.0;
                dc_forward_block(DcSerial{}, blk.data(), vec, sol);
                for (int i = 0; i < DC_NB; ++i) vec[i] = sol[i];
                dc_backward_block(DcSerial{}, blk.data(), vec, sol);
                for (int i = 0; i < DC_NB; ++i) X[(size_t)c * DC_LD + i] = sol[i];
            }
            double* out = ztile(P.diag(k));
            for (int i = 0; i < DC_NB; ++i) for (int j = 0; j <= i; ++j) out[i * DC_NB + j] = out[j * DC_NB + i] = X[(size_t)j * DC_LD + i];
        }
    }
    void diag(int k) {
        const int32_t c0 = P.col_ptr[(size_t)k], m = P.s_size(k);
        double* out = ztile(P.diag(k));
        for (int i = 0; i < DC_NB; ++i)
            for (int j = 0; j <= i; ++j) {
                double s = 0.0;
                for (int a = 0; a < m; ++a) {
                    const double* g = G.data() + (size_t)a * SC_TILE; const double* z = ztile(P.col_tile[(size_t)(c0 + a)]);
                    for (int x = 0; x < DC_NB; ++x) s += g[x * DC_NB + i] * z[x * DC_NB + j];
                }
                out[i * DC_NB + j] = out[j * DC_NB + i] = out[i * DC_NB + j] - s;
            }
    }
};
// Z [tiles][4096] from the factored tiles T
inline void sc_host_selected_inverse(const ScPlan& P, const double* T, double* Z) {
    ScSelHost H{P, T, Z};
    sc_selinv_steps(P, H);
}

// ---- serial host instantiation of the panel sweeps (sc_panel_steps) on the factored tiles T: W [panels x 64][nc] in place, T is only read.  The substitutions are the
// block routines of pgo_dense_math.hpp, per row (forward: DcHost::substitute_row, the panel's; backward: dc_backward_block, as ScSelHost::ginv), never a product with an
// inverse; every product sum is formed from zero in the walker's order and subtracted once.
struct ScPanelHost {
    const ScPlan& P; const double* T; double* W; int nc; const int32_t* first;
    std::vector<double> blk = std::vector<double>((size_t)DC_NB * DC_LD, 0.0), acc = std::vector<double>(SC_TILE, 0.0);
    double vec[DC_NB], sol[DC_NB];
    void load_diag(int k) { const double* t = T + (size_t)P.diag(k) * SC_TILE; for (int i = 0; i < DC_NB; ++i) for (int j = 0; j < DC_NB; ++j) blk[(size_t)i * DC_LD + j] = t[i * DC_NB + j]; }
    double* row(int p, int r) const { return W + ((size_t)p * DC_NB + r) * nc; }
    void pfwd(int k, int started) {
        load_diag(k);
        for (int p = 0; p < started; ++p) {
            std::fill(acc.begin(), acc.end(), 0.0);
            for (int32_t id = P.row_ptr[(size_t)k]; id < P.diag(k); ++id) {
                const int j = P.row_col[(size_t)id];
                if (j < first[p]) continue;
                const double* t = T + (size_t)id * SC_TILE;
                for (int r = 0; r < DC_NB; ++r) {
                    const double* w = row(p, r) + (size_t)j * DC_NB;
                    for (int c = 0; c < DC_NB; ++c) {
                        double s = acc[(size_t)r * DC_NB + c];
                        for (int kk = 0; kk < DC_NB; ++kk) s += w[kk] * t[c * DC_NB + kk];
                        acc[(size_t)r * DC_NB + c] = s;
                    }
                }
            }
            for (int r = 0; r < DC_NB; ++r) {
                double* w = row(p, r) + (size_t)k * DC_NB;
                for (int c = 0; c < DC_NB; ++c) w[c] -= acc[(size_t)r * DC_NB + c];
                DcHost::substitute_row(blk.data(), w);
            }
        }
    }
    void pbwd(int k, int panels) {
        load_diag(k);
        for (int p = 0; p < panels; ++p) {
            std::fill(acc.begin(), acc.end(), 0.0);
            for (int32_t e = P.col_ptr[(size_t)k]; e < P.col_ptr[(size_t)k + 1]; ++e) {
                const double* t = T + (size_t)P.col_tile[(size_t)e] * SC_TILE;
                for (int r = 0; r < DC_NB; ++r) {
                    const double* w = row(p, r) + (size_t)P.col_row[(size_t)e] * DC_NB;
                    for (int c = 0; c < DC_NB; ++c) {
                        double s = acc[(size_t)r * DC_NB + c];
                        for (int kk = 0; kk < DC_NB; ++kk) s += w[kk] * t[kk * DC_NB + c];
                        acc[(size_t)r * DC_NB + c] = s;
                    }
                }
            }
            for (int r = 0; r < DC_NB; ++r) {
                double* w = row(p, r) + (size_t)k * DC_NB;
                for (int c = 0; c < DC_NB; ++c) vec[c] = w[c] - acc[(size_t)r * DC_NB + c];
                dc_backward_block(DcSerial{}, blk.data(), vec, sol);
                for (int c = 0; c < DC_NB; ++c) w[c] = sol[c];
            }
        }
    }
};

// Solves A x = b for the symmetric positive definite n x n matrix `a` with the tile-sparse factorisation, row i at position pos[i] < n (a permutation of 0 .. n - 1;
// nullptr: the identity).  Returns false — and leaves x alone — when a pivot failed.  info8 (may be null): nt, tiles of the matrix, tiles of L, 0, bytes of the tile
// storage, launches of one factorisation, of one pair of sweeps, tile updates.
inline bool sc_host_solve(int n, const double* a, const double* b, const int32_t* pos, double* x, int64_t* info8) {
    const ScPlan P = sc_plan_matrix(n, a, pos);
    const int nc = P.nt * DC_NB;
    if (info8) { const int64_t v[8] = {P.nt, P.a_tiles, P.tiles(), 0, (int64_t)(P.tiles() * (int64_t)SC_TILE * 8), P.factor_launches(), P.solve_launches(), P.tile_updates()}; std::copy(v, v + 8, info8); }
    std::vector<double> T((size_t)P.tiles() * SC_TILE, 0.0), w((size_t)nc, 0.0), yv((size_t)nc, 0.0), xs((size_t)nc, 0.0);
    sc_fill_tiles(P, n, a, pos, T.data());
    for (int i = 0; i < n; ++i) w[(size_t)(pos ? pos[i] : i)] = b[i];
    ScHost H{P, T.data(), w.data(), yv.data(), xs.data()};
    sc_factor_steps(P, H);
    if (H.failed) return false;
    sc_solve_steps(P, H);
    for (int i = 0; i < n; ++i) x[i] = xs[(size_t)(pos ? pos[i] : i)];
    return true;
}
#endif

}  // namespace pgo
