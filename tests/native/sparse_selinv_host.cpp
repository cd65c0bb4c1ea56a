// Host side of the tile-sparse selected inverse (csrc/pgo_sparse_math.hpp: sc_selinv_steps, ScSelHost, the plan's counts; csrc/pgo_sparse_blocks.hpp: the gather of
// 6 x 6 blocks): Takahashi's recurrence on the tiles of the factor, run serially — what pgo_sparse_chol_selected_{inverse, info, blocks} do on the device.  Built as a
// shared object for tests/test_sparse_selinv_host.py (tests/test_gpu_sparse_selinv.py reads its plan counts and its host inverse), or — with -DSSH_MAIN — as a
// stand-alone program that checks itself: the form to run under -fsanitize=address,undefined.
#include <cmath>
#include <cstring>

#include "pgo_sparse_blocks.hpp"

namespace {
struct HostSel {
    int64_t N = 0; int used = 0; bool factored = false, selected = false;
    pgo::ScPlan P;
    std::vector<uint8_t> in_system; std::vector<int32_t> order, pos, hi, lo;
    std::vector<double> T, Z;
};
// records the walker's calls: op 0 ginv, 1 column, 2 diag, 3 inverses (k = -1)
struct Trace {
    std::vector<int32_t>* out;
    void inverses() { out->push_back(3); out->push_back(-1); }
    void ginv(int k) { out->push_back(0); out->push_back(k); }
    void column(int k) { out->push_back(1); out->push_back(k); }
    void diag(int k) { out->push_back(2); out->push_back(k); }
};
}  // namespace

extern "C" {
// the plan of a tile pattern given as m lower tiles (ti[e] > tj[e]; the diagonal is implied): s_size [nt], counts2 = selinv_launches(), selinv_products(); trace
// [2 x (3 nt + 1)]: (op, k) of every call of sc_selinv_steps; returns the number of calls
long long ssh_plan_counts(int nt, long long m, const int* ti, const int* tj, int* s_size, long long* counts2, int* trace) {
    std::vector<std::vector<int32_t>> below((size_t)nt);
    for (long long e = 0; e < m; ++e) below[(size_t)tj[e]].push_back(ti[e]);
    const pgo::ScPlan P = pgo::sc_symbolic(nt, std::move(below));
    for (int k = 0; k < nt; ++k) s_size[k] = P.s_size(k);
    counts2[0] = P.selinv_launches(); counts2[1] = P.selinv_products();
    std::vector<int32_t> t;
    Trace tr{&t};
    pgo::sc_selinv_steps(P, tr);
    std::copy(t.begin(), t.end(), trace);
    return (long long)(t.size() / 2);
}

// The selected inverse of the symmetric positive definite n x n matrix `a`, row i at position pos[i] (nullptr: where it is), through the matrix interface's plan
// (sc_plan_matrix).  sigma, mask [n][n] in the CALLER's order: the entries of the inverse whose tile is in the pattern of L (mask 1), 0 elsewhere.  info4: launches,
// tile products, bytes of Z, tiles of L.  Returns 1; 0: a pivot failed; -1: the padding rows did not come back as exactly 1 on the diagonal and 0 elsewhere, or a
// diagonal tile is not exactly symmetric.  x (may be nullptr) [n]: the solution of a x = b on the same factor AFTER the selected inverse (the factor survives).
int ssh_matrix(int n, const double* a, const int* pos, double* sigma, unsigned char* mask, long long* info4, const double* b, double* x) {
    const pgo::ScPlan P = pgo::sc_plan_matrix(n, a, pos);
    const int nc = P.nt * pgo::DC_NB;
    std::vector<double> T((size_t)P.tiles() * pgo::SC_TILE, 0.0), Z((size_t)P.tiles() * pgo::SC_TILE, 7.0);
    pgo::sc_fill_tiles(P, n, a, pos, T.data());
    pgo::ScHost H{P, T.data(), nullptr, nullptr, nullptr};
    pgo::sc_factor_steps(P, H);
    if (H.failed) return 0;
    pgo::sc_host_selected_inverse(P, T.data(), Z.data());
    const long long v[4] = {P.selinv_launches(), P.selinv_products(), (long long)(P.tiles() * (long long)pgo::SC_TILE * 8), P.tiles()};
    for (int k = 0; k < 4; ++k) info4[k] = v[k];
    auto at = [&](int r, int c) -> const double* {      // entry (r, c) of the permuted inverse, nullptr outside the pattern
        const int hi = std::max(r, c), lo = std::min(r, c), id = P.find(hi / pgo::DC_NB, lo / pgo::DC_NB);
        return id < 0 ? nullptr : &Z[(size_t)id * pgo::SC_TILE + (size_t)(hi % pgo::DC_NB) * pgo::DC_NB + lo % pgo::DC_NB];
    };
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            const double* p = at(pos ? pos[i] : i, pos ? pos[j] : j);
            sigma[(size_t)i * n + j] = p ? *p : 0.0; mask[(size_t)i * n + j] = p ? 1 : 0;
        }
    int rc = 1;
    for (int r = n; r < nc; ++r)      // padding: identity rows
        for (int c = 0; c < nc; ++c) { const double* p = at(r, c); if (p && *p != (r == c ? 1.0 : 0.0)) rc = -1; }
    for (int k = 0; k < P.nt; ++k) {      // both triangles of a diagonal tile, equal bits
        const double* t = &Z[(size_t)P.diag(k) * pgo::SC_TILE];
        for (int i = 0; i < pgo::DC_NB; ++i) for (int j = 0; j < i; ++j) if (std::memcmp(&t[i * pgo::DC_NB + j], &t[j * pgo::DC_NB + i], sizeof(double)) != 0) rc = -1;
    }
    if (x) {
        std::vector<double> w((size_t)nc, 0.0), yv((size_t)nc, 0.0), xs((size_t)nc, 0.0);
        for (int i = 0; i < n; ++i) w[(size_t)(pos ? pos[i] : i)] = b[i];
        pgo::ScHost S{P, T.data(), w.data(), yv.data(), xs.data()};
        pgo::sc_solve_steps(P, S);
        for (int i = 0; i < n; ++i) x[i] = xs[(size_t)(pos ? pos[i] : i)];
    }
    return rc;
}

// the block interface on the host: pgo_sparse_chol_{create, factor, selected_inverse, selected_info, selected_blocks}.  nullptr: the pair list is refused.
void* ssh_create(long long N, const unsigned char* in_system, long long n_pairs, const int* hi, const int* lo, int ordering) {
    if (pgo::sc_check_pairs(N, in_system, n_pairs, hi, lo)) return nullptr;
    HostSel* h = new HostSel;
    h->N = N; h->in_system.assign(in_system, in_system + N); h->hi.assign(hi, hi + n_pairs); h->lo.assign(lo, lo + n_pairs);
    std::vector<int64_t> adj_ptr; std::vector<int32_t> adj;
    pgo::sc_pair_adjacency(N, n_pairs, hi, lo, adj_ptr, adj);
    h->P = pgo::sc_plan_graph(N, adj_ptr.data(), adj.data(), in_system, ordering, h->order, &h->used);
    h->pos.assign((size_t)N, 0);
    for (long long q = 0; q < N; ++q) h->pos[(size_t)h->order[(size_t)q]] = (int32_t)q;
    return h;
}
void ssh_destroy(void* p) { delete static_cast<HostSel*>(p); }
// 1: factored; 0: a pivot failed.  Either way a selected inverse of an earlier factor is gone.
int ssh_factor(void* p, const double* diag, const double* blocks) {
    HostSel& h = *static_cast<HostSel*>(p);
    h.selected = false;
    h.T.assign((size_t)h.P.tiles() * pgo::SC_TILE, 0.0);
    pgo::sc_fill_blocks_host(h.P, h.N, h.in_system.data(), h.pos.data(), diag, (int64_t)h.hi.size(), h.hi.data(), h.lo.data(), blocks, h.T.data());
    pgo::ScHost H{h.P, h.T.data(), nullptr, nullptr, nullptr};
    pgo::sc_factor_steps(h.P, H);
    h.factored = !H.failed;
    return h.factored ? 1 : 0;
}
// 0: done; -5 (PGO_ERR_STATE): no factor
int ssh_selected_inverse(void* p) {
    HostSel& h = *static_cast<HostSel*>(p);
    if (!h.factored) return -5;
    h.Z.assign((size_t)h.P.tiles() * pgo::SC_TILE, 7.0);
    pgo::sc_host_selected_inverse(h.P, h.T.data(), h.Z.data());
    h.selected = true;
    return 0;
}
// info4 as pgo_sparse_chol_selected_info; order (may be nullptr) [N]; l_tiles
void ssh_info(void* p, long long* info4, int* order, long long* l_tiles) {
    const HostSel& h = *static_cast<HostSel*>(p);
    const long long v[4] = {h.P.selinv_launches(), h.P.selinv_products(), (long long)(h.P.tiles() * (long long)pgo::SC_TILE * 8), h.selected ? 1 : 0};
    for (int k = 0; k < 4; ++k) info4[k] = v[k];
    if (order) std::copy(h.order.begin(), h.order.end(), order);
    if (l_tiles) *l_tiles = h.P.tiles();
}
// 0: done; -5: no selected inverse; -1: a keyframe out of range
int ssh_selected_blocks(void* p, long long n_blocks, const int* na, const int* nb, double* out, unsigned char* in_pattern) {
    const HostSel& h = *static_cast<HostSel*>(p);
    for (long long k = 0; k < n_blocks; ++k) if (na[k] < 0 || na[k] >= h.N || nb[k] < 0 || nb[k] >= h.N) return -1;
    if (!h.selected) return -5;
    for (long long k = 0; k < n_blocks; ++k) in_pattern[k] = pgo::sc_selected_block_host(h.P, h.Z.data(), h.in_system.data(), h.pos.data(), na[k], nb[k], out + 36 * k) ? 1 : 0;
    return 0;
}
}

#ifdef SSH_MAIN
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
        std::vector<int> pos;
        if (c.permute) {      // a permutation of the 6-row nodes: node i to position (17 i + 5) mod nodes
            const int nodes = n / 6;
            pos.resize((size_t)n);
            for (int i = 0; i < nodes; ++i) for (int a = 0; a < 6; ++a) pos[(size_t)i * 6 + a] = ((17 * i + 5) % nodes) * 6 + a;
        }
        std::vector<double> S((size_t)n * n);
        std::vector<unsigned char> mask((size_t)n * n);
        long long info[4];
        const int rc = ssh_matrix(n, A.data(), c.permute ? pos.data() : nullptr, S.data(), mask.data(), info, nullptr, nullptr);
        if (rc != 1) { std::printf("%s: rc %d\n", c.name, rc); ++bad; continue; }
        // (A Sigma)_ij = delta_ij needs whole columns of Sigma; where column j of the pattern is full (every entry of row-set of A's column in the mask) check it
        double worst = 0.0; long long checked = 0;
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) {
                if (!mask[(size_t)i * n + j]) continue;
                bool whole = true;
                double r = i == j ? -1.0 : 0.0;
                for (int k = 0; k < n && whole; ++k) { if (A[(size_t)i * n + k] == 0.0) continue; if (!mask[(size_t)k * n + j]) whole = false; else r += A[(size_t)i * n + k] * S[(size_t)k * n + j]; }
                if (whole) { worst = std::fmax(worst, std::fabs(r)); ++checked; }
                if (S[(size_t)i * n + j] != S[(size_t)j * n + i]) { std::printf("%s: not symmetric at (%d, %d)\n", c.name, i, j); ++bad; i = j = n; }
            }
        std::printf("%s: n = %d, %lld tiles of L, %lld launches, %lld products, |A Sigma - I| <= %.3e over %lld entries\n", c.name, n, info[3], info[0], info[1], worst, checked);
        if (!(worst <= 1e-12) || checked == 0) ++bad;
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
            void* h = ssh_create(N, in.data(), np, hi.data(), lo.data(), ordering);
            if (!h) { std::printf("ordering %d: the pairs were refused\n", ordering); ++bad; continue; }
            const int na[6] = {10, 37, 2, 11, 0, 5}, nb[6] = {10, 2, 37, 3, 39, 30};
            std::vector<double> out((size_t)6 * 36, 7.0);
            unsigned char flag[6];
            if (ssh_selected_inverse(h) != -5) { std::printf("ordering %d: a selected inverse without a factor\n", ordering); ++bad; }
            if (!ssh_factor(h, diag.data(), blocks.data())) { std::printf("ordering %d: reported not positive definite\n", ordering); ++bad; ssh_destroy(h); continue; }
            if (ssh_selected_blocks(h, 6, na, nb, out.data(), flag) != -5) { std::printf("ordering %d: blocks without a selected inverse\n", ordering); ++bad; }
            if (ssh_selected_inverse(h) != 0 || ssh_selected_blocks(h, 6, na, nb, out.data(), flag) != 0) { std::printf("ordering %d: refused\n", ordering); ++bad; ssh_destroy(h); continue; }
            for (int a = 0; a < 6; ++a) for (int c = 0; c < 6; ++c) {
                if (out[(size_t)a * 6 + c] != out[(size_t)c * 6 + a]) { std::printf("ordering %d: the block of keyframe 10 is not symmetric\n", ordering); ++bad; a = c = 6; break; }
                if (out[36 + (size_t)a * 6 + c] != out[72 + (size_t)c * 6 + a]) { std::printf("ordering %d: (b, a) is not the transpose of (a, b)\n", ordering); ++bad; a = c = 6; break; }
            }
            for (int e = 0; e < 72; ++e) if (out[108 + (size_t)e] != 0.0) { std::printf("ordering %d: a keyframe outside the system gave a non-zero block\n", ordering); ++bad; break; }
            if (!flag[0] || !flag[1] || !flag[2] || !flag[3] || !flag[4]) { std::printf("ordering %d: a block of the system is reported out of the pattern\n", ordering); ++bad; }
            std::printf("ordering %d: var(keyframe 10, entry 0) = %.6e, the far pair (5, 30) in the pattern: %d\n", ordering, out[0], (int)flag[5]);
            if (!(out[0] > 0.0)) ++bad;
            if (!ssh_factor(h, diag.data(), blocks.data()) || ssh_selected_blocks(h, 6, na, nb, out.data(), flag) != -5) { std::printf("ordering %d: a new factor kept the selected inverse\n", ordering); ++bad; }
            const int oa[1] = {40}, ob[1] = {0};
            if (ssh_selected_blocks(h, 1, oa, ob, out.data(), flag) != -1) { std::printf("ordering %d: a keyframe out of range was accepted\n", ordering); ++bad; }
            ssh_destroy(h);
        }
    }
    std::printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}
#endif
