// Host side of the columns of the inverse in number (csrc/pgo_sparse_math.hpp: sc_panel_steps, ScPanelHost, ScPlan::panel_launches / panel_products;
// csrc/pgo_sparse_blocks.hpp: sc_column_chunks, ScColumns, the gather): both sweeps over panels of 64 right-hand sides on the tiles of the factor, run serially — what
// pgo_sparse_chol_inverse_columns does on the device.  Built as a shared object for tests/test_sparse_panel_host.py (tests/test_gpu_sparse_panel.py reads its counts
// and its host blocks), or — with -DSPH_MAIN — as a stand-alone program that checks itself: the form to run under -fsanitize=address,undefined.
#include <cmath>
#include <cstring>

#include "pgo_sparse_blocks.hpp"

namespace {
struct HostCols {
    int64_t N = 0; int used = 0; bool factored = false;
    pgo::ScPlan P;
    std::vector<uint8_t> in_system; std::vector<int32_t> order, pos, hi, lo;
    std::vector<double> T;
};
// records the walker's calls: (op, k, workgroups), op 0 pfwd, 1 pbwd
struct Trace {
    std::vector<int32_t>* out;
    void pfwd(int k, int started) { out->push_back(0); out->push_back(k); out->push_back(started); }
    void pbwd(int k, int panels) { out->push_back(1); out->push_back(k); out->push_back(panels); }
};
}  // namespace

extern "C" {
// the plan of a tile pattern given as m lower tiles (ti[e] > tj[e]; the diagonal is implied), panels with first[] ascending and k_stop: counts2 = panel_launches(),
// panel_products(); trace [3 x 2 nt]: (op, k, workgroups) of every call of sc_panel_steps; returns the number of calls
long long spp_plan_counts(int nt, long long m, const int* ti, const int* tj, int n_panels, const int* first, int k_stop, long long* counts2, int* trace) {
    std::vector<std::vector<int32_t>> below((size_t)nt);
    for (long long e = 0; e < m; ++e) below[(size_t)tj[e]].push_back(ti[e]);
    const pgo::ScPlan P = pgo::sc_symbolic(nt, std::move(below));
    const std::vector<int32_t> f(first, first + n_panels);
    counts2[0] = P.panel_launches(f.data(), n_panels, k_stop); counts2[1] = P.panel_products(f.data(), n_panels, k_stop);
    std::vector<int32_t> t;
    Trace tr{&t};
    pgo::sc_panel_steps(P, f, k_stop, tr);
    std::copy(t.begin(), t.end(), trace);
    return (long long)(t.size() / 3);
}

// runs of sc_column_chunks: bounds [2 x runs], room for n_cols runs; returns their number
long long spp_chunks(long long n_cols, int nc, long long workspace_bytes, long long* bounds) {
    const auto runs = pgo::sc_column_chunks(n_cols, nc, workspace_bytes);
    for (size_t r = 0; r < runs.size(); ++r) { bounds[2 * r] = runs[r].first; bounds[2 * r + 1] = runs[r].second; }
    return (long long)runs.size();
}

// The columns cols[0 .. m) (the caller's indices, any order) of the inverse of the symmetric positive definite n x n matrix `a`, row i at position pos[i] (nullptr:
// where it is), through the matrix interface's plan (sc_plan_matrix): unit rows sorted by position into panels, both sweeps, the backward one down to tile k_stop.
// X [m][n]: column cols[r] in the caller's order — its entries at positions below 64 k_stop are not solutions.  Xs (may be nullptr) [m][n]: the same columns from the
// two sweeps of ScHost, one right-hand side at a time.  info2: launches of the sweeps, tile products.  Returns 1; 0: a pivot failed.
int spp_matrix(int n, const double* a, const int* pos, int m, const int* cols, int k_stop, double* X, double* Xs, long long* info2) {
    const pgo::ScPlan P = pgo::sc_plan_matrix(n, a, pos);
    const int nc = P.nt * pgo::DC_NB;
    std::vector<double> T((size_t)P.tiles() * pgo::SC_TILE, 0.0);
    pgo::sc_fill_tiles(P, n, a, pos, T.data());
    pgo::ScHost H{P, T.data(), nullptr, nullptr, nullptr};
    pgo::sc_factor_steps(P, H);
    if (H.failed) return 0;
    std::vector<int> by(m);
    for (int r = 0; r < m; ++r) by[(size_t)r] = r;
    std::sort(by.begin(), by.end(), [&](int x, int y) { return (pos ? pos[cols[x]] : cols[x]) < (pos ? pos[cols[y]] : cols[y]); });
    const int m_pad = (m + pgo::DC_NB - 1) / pgo::DC_NB * pgo::DC_NB;
    std::vector<double> W((size_t)m_pad * nc, 0.0);
    std::vector<int32_t> first;
    for (int r = 0; r < m; ++r) {
        const int c = pos ? pos[cols[by[(size_t)r]]] : cols[by[(size_t)r]];
        W[(size_t)r * nc + c] = 1.0;
        if (r % pgo::DC_NB == 0) first.push_back(c / pgo::DC_NB);
    }
    pgo::ScPanelHost S{P, T.data(), W.data(), nc, first.data()};
    pgo::sc_panel_steps(P, first, k_stop, S);
    info2[0] = P.panel_launches(first.data(), (int)first.size(), k_stop); info2[1] = P.panel_products(first.data(), (int)first.size(), k_stop);
    for (int r = 0; r < m; ++r)
        for (int i = 0; i < n; ++i) X[(size_t)by[(size_t)r] * n + i] = W[(size_t)r * nc + (pos ? pos[i] : i)];
    if (Xs) {
        std::vector<double> w((size_t)nc), yv((size_t)nc), xs((size_t)nc);
        for (int r = 0; r < m; ++r) {
            std::fill(w.begin(), w.end(), 0.0); std::fill(yv.begin(), yv.end(), 0.0); std::fill(xs.begin(), xs.end(), 0.0);
            w[(size_t)(pos ? pos[cols[r]] : cols[r])] = 1.0;
            pgo::ScHost V{P, T.data(), w.data(), yv.data(), xs.data()};
            pgo::sc_solve_steps(P, V);
            for (int i = 0; i < n; ++i) Xs[(size_t)r * n + i] = xs[(size_t)(pos ? pos[i] : i)];
        }
    }
    return 1;
}

// the block interface on the host: pgo_sparse_chol_{create, factor, inverse_columns}.  nullptr: the pair list is refused.
void* spp_create(long long N, const unsigned char* in_system, long long n_pairs, const int* hi, const int* lo, int ordering) {
    if (pgo::sc_check_pairs(N, in_system, n_pairs, hi, lo)) return nullptr;
    HostCols* h = new HostCols;
    h->N = N; h->in_system.assign(in_system, in_system + N); h->hi.assign(hi, hi + n_pairs); h->lo.assign(lo, lo + n_pairs);
    std::vector<int64_t> adj_ptr; std::vector<int32_t> adj;
    pgo::sc_pair_adjacency(N, n_pairs, hi, lo, adj_ptr, adj);
    h->P = pgo::sc_plan_graph(N, adj_ptr.data(), adj.data(), in_system, ordering, h->order, &h->used);
    h->pos.assign((size_t)N, 0);
    for (long long q = 0; q < N; ++q) h->pos[(size_t)h->order[(size_t)q]] = (int32_t)q;
    return h;
}
void spp_destroy(void* p) { delete static_cast<HostCols*>(p); }
// order (may be nullptr) [N]; returns nt
int spp_info(void* p, int* order) {
    const HostCols& h = *static_cast<HostCols*>(p);
    if (order) std::copy(h.order.begin(), h.order.end(), order);
    return h.P.nt;
}
// 1: factored; 0: a pivot failed
int spp_factor(void* p, const double* diag, const double* blocks) {
    HostCols& h = *static_cast<HostCols*>(p);
    h.T.assign((size_t)h.P.tiles() * pgo::SC_TILE, 0.0);
    pgo::sc_fill_blocks_host(h.P, h.N, h.in_system.data(), h.pos.data(), diag, (int64_t)h.hi.size(), h.hi.data(), h.lo.data(), blocks, h.T.data());
    pgo::ScHost H{h.P, h.T.data(), nullptr, nullptr, nullptr};
    pgo::sc_factor_steps(h.P, H);
    h.factored = !H.failed;
    return h.factored ? 1 : 0;
}
// 0: done; -5 (PGO_ERR_STATE): no factor; -1 (PGO_ERR_INVALID_ARG), out untouched: what ScColumns refuses.  info4: launches, tile products, workspace bytes, chunks
int spp_inverse_columns(void* p, long long n_cols, const int* col_node, long long n_blocks, const int* row_node, const int* col_index, long long workspace_bytes, double* out, long long* info4) {
    const HostCols& h = *static_cast<HostCols*>(p);
    if (!h.factored) return -5;
    const pgo::ScColumns Q(h.P, h.N, h.in_system.data(), h.pos.data(), n_cols, col_node, n_blocks, row_node, col_index, workspace_bytes);
    if (Q.error) return -1;
    const long long v[4] = {Q.launches, Q.products, Q.workspace, (long long)Q.chunks.size()};
    for (int k = 0; k < 4; ++k) info4[k] = v[k];
    pgo::sc_host_inverse_columns(h.P, h.T.data(), Q, h.in_system.data(), h.pos.data(), n_blocks, row_node, col_index, out);
    return 0;
}
// X = A^-1 B by ScHost's two sweeps, rows of B and X in the caller's keyframe order (pgo_sparse_chol_solve)
void spp_solve(void* p, long long n_rhs, const double* B, double* X) {
    const HostCols& h = *static_cast<HostCols*>(p);
    const int nc = h.P.nt * pgo::DC_NB;
    const size_t n6 = (size_t)h.N * 6;
    std::vector<double> w((size_t)nc), yv((size_t)nc), xs((size_t)nc);
    for (long long r = 0; r < n_rhs; ++r) {
        std::fill(w.begin(), w.end(), 0.0); std::fill(yv.begin(), yv.end(), 0.0); std::fill(xs.begin(), xs.end(), 0.0);
        for (long long i = 0; i < h.N; ++i) if (h.in_system[(size_t)i]) std::memcpy(&w[(size_t)h.pos[(size_t)i] * 6], B + (size_t)r * n6 + (size_t)i * 6, 6 * sizeof(double));
        pgo::ScHost V{h.P, const_cast<double*>(h.T.data()), w.data(), yv.data(), xs.data()};
        pgo::sc_solve_steps(h.P, V);
        for (long long i = 0; i < h.N; ++i)
            for (int a = 0; a < 6; ++a) X[(size_t)r * n6 + (size_t)i * 6 + a] = h.in_system[(size_t)i] ? xs[(size_t)h.pos[(size_t)i] * 6 + a] : 0.0;
    }
}
}

#ifdef SPH_MAIN
#include <cstdio>

static double lcg(unsigned long long& s) { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return (double)((s >> 11) & ((1ULL << 53) - 1)) / (double)(1ULL << 53) - 0.5; }

// a symmetric positive definite matrix whose tile pattern is `tiles` (pairs of tile row > tile column) plus the diagonal: random entries, a dominant diagonal
static std::vector<double> patterned(int n, const std::vector<std::pair<int, int>>& tiles, unsigned long long seed) {
    std::vector<double> A((size_t)n * n, 0.0);
    unsigned long long s = seed;
    auto fill = [&](int ti, int tj) {
        for (int i = ti * 64; i < std::min(n, ti * 64 + 64); ++i)
            for (int j = tj * 64; j < std::min(n, tj * 64 + 64); ++j) { if (j >= i) continue; const double v = lcg(s); A[(size_t)i * n + j] = v; A[(size_t)j * n + i] = v; }
    };
    for (int t = 0; t * 64 < n; ++t) fill(t, t);
    for (const auto& t : tiles) fill(t.first, t.second);
    for (int i = 0; i < n; ++i) { double r = 0.0; for (int j = 0; j < n; ++j) r += std::fabs(A[(size_t)i * n + j]); A[(size_t)i * n + i] = r + 1.0; }
    return A;
}

int main() {
    int bad = 0;
    struct Case { const char* name; int n; std::vector<std::pair<int, int>> tiles; bool permute; };
    const std::vector<Case> cases = {
        {"one tile", 64, {}, false}, {"padding", 96, {{1, 0}}, false}, {"block diagonal", 128, {}, false}, {"arrow", 320, {{4, 0}, {4, 1}, {4, 2}, {4, 3}}, false},
        {"fill", 192, {{1, 0}, {2, 0}}, false}, {"gap", 320, {{2, 0}, {4, 0}}, false}, {"band, two wide", 200, {{1, 0}, {2, 1}, {3, 2}, {2, 0}, {3, 1}}, false},
        {"arrow, permuted", 318, {{4, 0}, {4, 1}, {4, 2}, {4, 3}}, true},
    };
    for (const Case& c : cases) {
        const int n = c.n;
        const std::vector<double> A = patterned(n, c.tiles, 99ULL + (unsigned long long)n);
        std::vector<int> pos, cols((size_t)n);
        if (c.permute) {      // a permutation of the 6-row nodes: node i to position (17 i + 5) mod nodes
            const int nodes = n / 6;
            pos.resize((size_t)n);
            for (int i = 0; i < nodes; ++i) for (int a = 0; a < 6; ++a) pos[(size_t)i * 6 + a] = ((17 * i + 5) % nodes) * 6 + a;
        }
        for (int i = 0; i < n; ++i) cols[(size_t)i] = n - 1 - i;      // (any order: the shim sorts them by position)
        std::vector<double> X((size_t)n * n), Xs((size_t)n * n);
        long long info[2];
        if (spp_matrix(n, A.data(), c.permute ? pos.data() : nullptr, n, cols.data(), 0, X.data(), Xs.data(), info) != 1) { std::printf("%s: a pivot failed\n", c.name); ++bad; continue; }
        double worst = 0.0, apart = 0.0;
        for (int r = 0; r < n; ++r)
            for (int i = 0; i < n; ++i) {
                double s = i == cols[(size_t)r] ? -1.0 : 0.0;
                for (int k = 0; k < n; ++k) s += A[(size_t)i * n + k] * X[(size_t)r * n + k];
                worst = std::fmax(worst, std::fabs(s));
                apart = std::fmax(apart, std::fabs(X[(size_t)r * n + i] - Xs[(size_t)r * n + i]));
            }
        std::printf("%s: n = %d, %lld launches, %lld products, |A X - I| <= %.3e, against the two sweeps %.3e\n", c.name, n, info[0], info[1], worst, apart);
        if (!(worst <= 1e-12) || !(apart <= 1e-12)) ++bad;
    }
    {   // the block interface: a chain of 40 keyframes with two loop closures, keyframes 11 and 39 outside the system
        const long long N = 40;
        std::vector<unsigned char> in((size_t)N, 1); in[11] = in[39] = 0;
        std::vector<int> hi, lo;
        for (int i = 0; i + 1 < N; ++i) if (in[(size_t)i] && in[(size_t)i + 1]) { hi.push_back(i % 2 ? i : i + 1); lo.push_back(i % 2 ? i + 1 : i); }
        hi.push_back(37); lo.push_back(2); hi.push_back(10); lo.push_back(12);
        const long long np = (long long)hi.size();
        unsigned long long s = 5ULL;
        std::vector<double> diag((size_t)N * 36, 0.0), blocks((size_t)np * 36);
        for (double& v : blocks) v = lcg(s);
        for (long long i = 0; i < N; ++i) for (int a = 0; a < 6; ++a) for (int c = 0; c <= a; ++c) { const double v = a == c ? 30.0 + lcg(s) : lcg(s); diag[(size_t)i * 36 + a * 6 + c] = diag[(size_t)i * 36 + c * 6 + a] = v; }
        for (int ordering : {0, 1}) {
            void* h = spp_create(N, in.data(), np, hi.data(), lo.data(), ordering);
            if (!h) { std::printf("ordering %d: the pairs were refused\n", ordering); ++bad; continue; }
            const int nt = spp_info(h, nullptr);
            const long long big = 1LL << 30, one_panel = 64LL * 64 * nt * 8;
            std::vector<int> colsv((size_t)N), rows, cidx;
            for (int i = 0; i < N; ++i) colsv[(size_t)i] = i;
            for (int a = 0; a < N; ++a) for (int b = 0; b < N; ++b) { rows.push_back(a); cidx.push_back(b); }
            const long long nb = (long long)rows.size();
            std::vector<double> all((size_t)nb * 36, 7.0), chunked((size_t)nb * 36, 7.0), alone(36, 7.0);
            long long info[4], info_c[4], info_1[4];
            if (spp_inverse_columns(h, N, colsv.data(), nb, rows.data(), cidx.data(), big, all.data(), info) != -5) { std::printf("ordering %d: columns without a factor\n", ordering); ++bad; }
            if (!spp_factor(h, diag.data(), blocks.data())) { std::printf("ordering %d: reported not positive definite\n", ordering); ++bad; spp_destroy(h); continue; }
            if (spp_inverse_columns(h, N, colsv.data(), nb, rows.data(), cidx.data(), big, all.data(), info) != 0 ||
                spp_inverse_columns(h, N, colsv.data(), nb, rows.data(), cidx.data(), one_panel, chunked.data(), info_c) != 0) { std::printf("ordering %d: refused\n", ordering); ++bad; spp_destroy(h); continue; }
            const int c10[1] = {10}, r5[1] = {5}, z[1] = {0};
            if (spp_inverse_columns(h, 1, c10, 1, r5, z, big, alone.data(), info_1) != 0) { std::printf("ordering %d: one block refused\n", ordering); ++bad; }
            if (std::memcmp(all.data(), chunked.data(), all.size() * sizeof(double)) != 0 || info_c[3] < 3) { std::printf("ordering %d: %lld chunks give other bits than one\n", ordering, info_c[3]); ++bad; }
            if (std::memcmp(alone.data(), &all[(size_t)(5 * N + 10) * 36], 36 * sizeof(double)) != 0) { std::printf("ordering %d: block (5, 10) alone has other bits than in the batch\n", ordering); ++bad; }
            double asym = 0.0;
            for (int a = 0; a < N; ++a)
                for (int b = 0; b < N; ++b)
                    for (int i = 0; i < 6; ++i)
                        for (int j = 0; j < 6; ++j) {
                            const double v = all[(size_t)(a * N + b) * 36 + i * 6 + j], w = all[(size_t)(b * N + a) * 36 + j * 6 + i];
                            if (!in[(size_t)a] || !in[(size_t)b]) { if (v != 0.0) { std::printf("ordering %d: a keyframe outside the system gave a non-zero block\n", ordering); ++bad; a = b = (int)N; i = j = 6; } }
                            else asym = std::fmax(asym, std::fabs(v - w));
                        }
            std::printf("ordering %d: %lld launches, %lld products, %lld bytes; in %lld chunks %lld launches; var(keyframe 10, entry 0) = %.6e, |Sigma - Sigma^T| <= %.3e\n", ordering, info[0], info[1], info[2],
                        info_c[3], info_c[0], all[(size_t)(10 * N + 10) * 36], asym);
            if (!(all[(size_t)(10 * N + 10) * 36] > 0.0) || !(asym <= 1e-14)) ++bad;
            std::vector<double> keep(36, 7.0);
            const int out_of_range[1] = {40}, twice[2] = {3, 3}, idx1[1] = {1};
            if (spp_inverse_columns(h, 1, out_of_range, 1, r5, z, big, keep.data(), info_1) != -1 || spp_inverse_columns(h, 1, c10, 1, out_of_range, z, big, keep.data(), info_1) != -1 ||
                spp_inverse_columns(h, 2, twice, 1, r5, z, big, keep.data(), info_1) != -1 || spp_inverse_columns(h, 1, c10, 1, r5, idx1, big, keep.data(), info_1) != -1 ||
                spp_inverse_columns(h, 1, c10, 1, r5, z, one_panel - 1, keep.data(), info_1) != -1) { std::printf("ordering %d: a bad argument was accepted\n", ordering); ++bad; }
            for (double v : keep) if (v != 7.0) { std::printf("ordering %d: a refused call wrote to out\n", ordering); ++bad; break; }
            spp_destroy(h);
        }
    }
    std::printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}
#endif
