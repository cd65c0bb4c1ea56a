// Host side of the tile-sparse Cholesky solver (csrc/pgo_sparse_math.hpp): the orderings, the symbolic factorisation and the serial instantiation of the factor and the
// solve, in its order of block steps and with the dense solver's block routines.  Built as a shared object for tests/test_sparse_cholesky_host.py,
// or — with -DSCH_MAIN — as a stand-alone program that plans and solves a few systems (padding, an empty column structure, fill, a permutation, an indefinite matrix, a
// NaN) and checks them itself: the form to run under -fsanitize=address,undefined.
#include "pgo_sparse_math.hpp"

namespace {
// the plan's pattern of L by its row lists and by its column lists (nt x nt bytes each, lower triangle); returns the number of inconsistencies: a pair (a >= b) of some s_k
// that resolves to no tile, a column entry whose tile id is not the one the row list gives
int64_t export_plan(const pgo::ScPlan& P, uint8_t* by_row, uint8_t* by_col) {
    const int nt = P.nt;
    int64_t bad = 0;
    for (int i = 0; i < nt; ++i) {
        for (int32_t id = P.row_ptr[(size_t)i]; id < P.row_ptr[(size_t)i + 1]; ++id) by_row[(size_t)i * nt + P.row_col[(size_t)id]] = 1;
        if (P.row_col[(size_t)P.diag(i)] != i) ++bad;
    }
    for (int k = 0; k < nt; ++k) {
        by_col[(size_t)k * nt + k] = 1;
        const int32_t c0 = P.col_ptr[(size_t)k], m = P.s_size(k);
        for (int a = 0; a < m; ++a) {
            by_col[(size_t)P.col_row[(size_t)(c0 + a)] * nt + k] = 1;
            if (P.find(P.col_row[(size_t)(c0 + a)], k) != P.col_tile[(size_t)(c0 + a)]) ++bad;
            if (a > 0 && P.col_row[(size_t)(c0 + a)] <= P.col_row[(size_t)(c0 + a - 1)]) ++bad;
            for (int b = 0; b <= a; ++b) if (P.find(P.col_row[(size_t)(c0 + a)], P.col_row[(size_t)(c0 + b)]) < 0) ++bad;
        }
        if ((P.ahead[(size_t)k] != 0) != (m > 0 && P.col_row[(size_t)c0] == k + 1)) ++bad;
    }
    return bad;
}
void export_info(const pgo::ScPlan& P, int used, int64_t* info8) {
    const int64_t v[8] = {P.nt, P.a_tiles, P.tiles(), used, (int64_t)(P.tiles() * (int64_t)pgo::SC_TILE * 8), P.factor_launches(), P.solve_launches(), P.tile_updates()};
    for (int k = 0; k < 8; ++k) info8[k] = v[k];
}
}  // namespace

extern "C" {
// symbolic factorisation of a tile pattern given as m lower tiles (ti[e] > tj[e]; the diagonal is implied); by_row, by_col: zeroed nt x nt
int64_t sch_symbolic(int nt, int64_t m, const int32_t* ti, const int32_t* tj, uint8_t* by_row, uint8_t* by_col, int64_t* info8) {
    std::vector<std::vector<int32_t>> below((size_t)nt);
    for (int64_t e = 0; e < m; ++e) below[(size_t)tj[e]].push_back(ti[e]);
    const pgo::ScPlan P = pgo::sc_symbolic(nt, std::move(below));
    export_info(P, 0, info8);
    return export_plan(P, by_row, by_col);
}
// ordering + plan of a graph (adjacency in CSR form); order_out [N]
int64_t sch_graph_plan(int64_t N, const int64_t* adj_ptr, const int32_t* adj, const uint8_t* in_system, int ordering, int32_t* order_out, uint8_t* by_row, uint8_t* by_col, int64_t* info8) {
    std::vector<int32_t> order;
    int used = 0;
    const pgo::ScPlan P = pgo::sc_plan_graph(N, adj_ptr, adj, in_system, ordering, order, &used);
    for (int64_t q = 0; q < N; ++q) order_out[q] = order[(size_t)q];
    export_info(P, used, info8);
    return export_plan(P, by_row, by_col);
}
int sch_nt_of(int64_t N) { const int n = (int)((N * 6 + pgo::DC_NB - 1) / pgo::DC_NB * pgo::DC_NB); return (n < pgo::DC_NB ? pgo::DC_NB : n) / pgo::DC_NB; }
// 1: solved; 0: a pivot was not positive (x untouched).  pos: nullptr, or the position of every row (a permutation of 0 .. n - 1)
int sch_solve(int n, const double* a, const double* b, const int32_t* pos, double* x, int64_t* info8) { return pgo::sc_host_solve(n, a, b, pos, x, info8) ? 1 : 0; }
// the dense solver's host instantiation on the same system
int sch_dense_solve(int n, const double* a, const double* b, double* x) { return pgo::dc_host_solve(n, a, b, x) ? 1 : 0; }
}

#ifdef SCH_MAIN
#include <cstdio>
#include <cstring>
#include <limits>

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
        {"fill", 192, {{1, 0}, {2, 0}}, false}, {"band", 384, {{1, 0}, {2, 1}, {3, 2}, {4, 3}, {5, 4}}, false}, {"full", 200, {{1, 0}, {2, 0}, {3, 0}, {2, 1}, {3, 1}, {3, 2}}, false},
        {"arrow, permuted", 318, {{4, 0}, {4, 1}, {4, 2}, {4, 3}}, true},
    };
    for (const Case& c : cases) {
        const int n = c.n;
        const std::vector<double> A = patterned(n, c.tiles, 99ULL + (unsigned long long)n);
        unsigned long long s = 7ULL + (unsigned long long)n;
        std::vector<double> b((size_t)n), x((size_t)n, 0.0), xd((size_t)n, 0.0);
        for (double& v : b) v = lcg(s);
        std::vector<int32_t> pos;
        if (c.permute) {      // a permutation of the 6-row nodes: node i to position (17 i + 5) mod nodes
            const int nodes = n / 6;
            pos.resize((size_t)n);
            for (int i = 0; i < nodes; ++i) for (int a = 0; a < 6; ++a) pos[(size_t)i * 6 + a] = ((17 * i + 5) % nodes) * 6 + a;
        }
        int64_t info[8];
        if (!sch_solve(n, A.data(), b.data(), c.permute ? pos.data() : nullptr, x.data(), info)) { std::printf("%s: reported not positive definite\n", c.name); ++bad; continue; }
        double rmax = 0.0, anorm = 0.0, xmax = 0.0, bmax = 0.0;
        for (int i = 0; i < n; ++i) {
            double r = b[(size_t)i], rowsum = 0.0;
            for (int j = 0; j < n; ++j) { r -= A[(size_t)i * n + j] * x[(size_t)j]; rowsum += std::fabs(A[(size_t)i * n + j]); }
            rmax = std::fmax(rmax, std::fabs(r)); anorm = std::fmax(anorm, rowsum); xmax = std::fmax(xmax, std::fabs(x[(size_t)i])); bmax = std::fmax(bmax, std::fabs(b[(size_t)i]));
        }
        const double eta = rmax / (anorm * xmax + bmax), bound = 2.0 * n * std::numeric_limits<double>::epsilon() / 2.0;      // (n u for the solve + n u for this residual's own rounding)
        std::printf("%s: n = %d, %lld tiles of L, eta = %.3e (bound %.3e)\n", c.name, n, (long long)info[2], eta, bound);
        if (!(eta <= bound)) ++bad;
        if (!c.permute) {      // natural order: the dense solver's numbers
            if (!sch_dense_solve(n, A.data(), b.data(), xd.data())) { std::printf("%s: the dense solver reported a failed pivot\n", c.name); ++bad; continue; }
            for (int i = 0; i < n; ++i) if (!(x[(size_t)i] == xd[(size_t)i])) { std::printf("%s: entry %d differs from the dense solver's\n", c.name, i); ++bad; break; }
        }
    }
    {
        std::vector<double> A((size_t)128 * 128, 0.0), b(128, 1.0), x(128, 7.0);
        for (int i = 0; i < 128; ++i) A[(size_t)i * 128 + i] = 1.0;
        A[(size_t)70 * 128 + 70] = -1.0;
        if (sch_solve(128, A.data(), b.data(), nullptr, x.data(), nullptr) || x[0] != 7.0) { std::printf("indefinite matrix: not reported\n"); ++bad; }
        A[(size_t)70 * 128 + 70] = 1.0;
        A[(size_t)100 * 128 + 3] = A[(size_t)3 * 128 + 100] = std::numeric_limits<double>::quiet_NaN();
        if (sch_solve(128, A.data(), b.data(), nullptr, x.data(), nullptr)) { std::printf("NaN: not reported\n"); ++bad; }
    }
    {      // a chain of 40 keyframes with one loop closure and two keyframes outside the system: both orders are permutations, the outsiders go last under RCM
        const int64_t N = 40;
        std::vector<std::vector<int32_t>> nb((size_t)N);
        auto edge = [&](int a, int b) { nb[(size_t)a].push_back(b); nb[(size_t)b].push_back(a); };
        for (int i = 0; i + 1 < N; ++i) edge(i, i + 1);
        edge(2, 37);
        std::vector<int64_t> ptr(1, 0); std::vector<int32_t> adj;
        for (const auto& v : nb) { adj.insert(adj.end(), v.begin(), v.end()); ptr.push_back((int64_t)adj.size()); }
        std::vector<uint8_t> in_system((size_t)N, 1); in_system[11] = in_system[39] = 0;
        const int nt = sch_nt_of(N);
        for (int ordering : {-1, 0, 1}) {
            std::vector<int32_t> order((size_t)N); std::vector<uint8_t> r((size_t)nt * nt, 0), c((size_t)nt * nt, 0); int64_t info[8];
            if (sch_graph_plan(N, ptr.data(), adj.data(), in_system.data(), ordering, order.data(), r.data(), c.data(), info) != 0 || std::memcmp(r.data(), c.data(), r.size()) != 0) { std::printf("graph plan, ordering %d: inconsistent\n", ordering); ++bad; }
            std::vector<int32_t> sorted(order); std::sort(sorted.begin(), sorted.end());
            for (int64_t i = 0; i < N; ++i) if (sorted[(size_t)i] != i) { std::printf("ordering %d: not a permutation\n", ordering); ++bad; break; }
            if (info[3] == 1 && !(order[(size_t)N - 2] == 11 && order[(size_t)N - 1] == 39)) { std::printf("RCM: the keyframes outside the system are not last\n"); ++bad; }
        }
    }
    std::printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}
#endif
