// Host side of libpgo_sparse.so (csrc/pgo_sparse_blocks.hpp on top of csrc/pgo_sparse_math.hpp): the reduction of a handle's normal blocks to the Schur complement's
// blocks, the checks of a pair list, the fill of the permuted tile matrix from 6 x 6 blocks, the right-hand sides of the inverse blocks — and, with ScHost, the whole
// block interface run serially: what pgo_sparse_chol_{create, factor, solve, inverse_blocks} do on the device.  Built as a shared object for
// tests/test_sparse_companion_host.py (tests/test_gpu_sparse_cholesky.py reads its plan figures and its host covariance), or — with -DSPH_MAIN — as a stand-alone
// program that checks itself: the form to run under -fsanitize=address,undefined.
#include <cmath>
#include <cstring>

#include "pgo_sparse_blocks.hpp"

namespace {
struct HostChol {
    int64_t N = 0; int used = 0; bool factored = false;
    pgo::ScPlan P;
    std::vector<uint8_t> in_system; std::vector<int32_t> order, pos, hi, lo;
    std::vector<double> T;
    int nc() const { return P.nt * pgo::DC_NB; }
};
}  // namespace

extern "C" {
// as pgo_sparse_reduce_normal_blocks
long long sph_reduce(long long N, const unsigned char* node_free, const double* diag, const double* offdiag, const double* sw_c, const double* sw_h, long long n_rel, const int* rc1, const int* rc2,
                     long long n_sw, const int* sc1, const int* sc2, int* pair_hi, int* pair_lo, double* s_diag, double* s_blocks) {
    const pgo::ScReduced R = pgo::sc_reduce_normal_blocks(N, node_free, diag, offdiag, sw_c, sw_h, n_rel, rc1, rc2, n_sw, sc1, sc2);
    std::copy(R.pair_hi.begin(), R.pair_hi.end(), pair_hi); std::copy(R.pair_lo.begin(), R.pair_lo.end(), pair_lo);
    std::copy(R.diag.begin(), R.diag.end(), s_diag); std::copy(R.blocks.begin(), R.blocks.end(), s_blocks);
    return (long long)R.pair_hi.size();
}
// sc_host_solve and dc_host_solve on a dense matrix: 1 solved, 0 a pivot failed
int sph_spd_solve(int n, const double* a, const double* b, const int* pos, double* x, long long* info8) {
    int64_t info[8];
    const bool ok = pgo::sc_host_solve(n, a, b, pos, x, info);
    for (int k = 0; k < 8; ++k) info8[k] = info[k];
    return ok ? 1 : 0;
}
int sph_dense_solve(int n, const double* a, const double* b, double* x) { return pgo::dc_host_solve(n, a, b, x) ? 1 : 0; }

// the block interface on the host.  nullptr: the pair list is refused.
void* sph_create(long long N, const unsigned char* in_system, long long n_pairs, const int* hi, const int* lo, int ordering) {
    if (pgo::sc_check_pairs(N, in_system, n_pairs, hi, lo)) return nullptr;
    HostChol* h = new HostChol;
    h->N = N; h->in_system.assign(in_system, in_system + N); h->hi.assign(hi, hi + n_pairs); h->lo.assign(lo, lo + n_pairs);
    std::vector<int64_t> adj_ptr; std::vector<int32_t> adj;
    pgo::sc_pair_adjacency(N, n_pairs, hi, lo, adj_ptr, adj);
    h->P = pgo::sc_plan_graph(N, adj_ptr.data(), adj.data(), in_system, ordering, h->order, &h->used);
    h->pos.assign((size_t)N, 0);
    for (long long q = 0; q < N; ++q) h->pos[(size_t)h->order[(size_t)q]] = (int32_t)q;
    return h;
}
void sph_destroy(void* p) { delete static_cast<HostChol*>(p); }
void sph_info(void* p, long long* info8, int* order) {
    const HostChol& h = *static_cast<HostChol*>(p);
    const long long v[8] = {h.P.nt, h.P.a_tiles, h.P.tiles(), h.used, (long long)(h.P.tiles() * (long long)pgo::SC_TILE * 8), h.P.factor_launches(), h.P.solve_launches(), h.P.tile_updates()};
    for (int k = 0; k < 8; ++k) info8[k] = v[k];
    if (order) std::copy(h.order.begin(), h.order.end(), order);
}
// 1: factored; 0: a pivot failed
int sph_factor(void* p, const double* diag, const double* blocks) {
    HostChol& h = *static_cast<HostChol*>(p);
    h.T.assign((size_t)h.P.tiles() * pgo::SC_TILE, 0.0);
    pgo::sc_fill_blocks_host(h.P, h.N, h.in_system.data(), h.pos.data(), diag, (int64_t)h.hi.size(), h.hi.data(), h.lo.data(), blocks, h.T.data());
    pgo::ScHost H{h.P, h.T.data(), nullptr, nullptr, nullptr};
    pgo::sc_factor_steps(h.P, H);
    h.factored = !H.failed;
    return h.factored ? 1 : 0;
}
void sph_solve(void* p, long long n_rhs, const double* B, double* X) {
    HostChol& h = *static_cast<HostChol*>(p);
    const size_t nc = (size_t)h.nc(), n6 = (size_t)h.N * 6;
    std::vector<double> w(nc), yv(nc), xs(nc);
    for (long long r = 0; r < n_rhs; ++r) {
        std::fill(w.begin(), w.end(), 0.0);
        for (long long i = 0; i < h.N; ++i) if (h.in_system[(size_t)i]) std::memcpy(&w[(size_t)h.pos[(size_t)i] * 6], B + (size_t)r * n6 + (size_t)i * 6, 6 * sizeof(double));
        pgo::ScHost H{h.P, h.T.data(), w.data(), yv.data(), xs.data()};
        pgo::sc_solve_steps(h.P, H);
        for (long long i = 0; i < h.N; ++i)
            for (int a = 0; a < 6; ++a) X[(size_t)r * n6 + (size_t)i * 6 + a] = h.in_system[(size_t)i] ? xs[(size_t)h.pos[(size_t)i] * 6 + a] : 0.0;
    }
}
// 0: done; -1: the rows are refused.  skip = 0: the forward sweep from tile 0 (the same bits)
int sph_inverse_blocks(void* p, long long n_groups, const long long* group_ptr, const long long* row_ptr, const int* col, const double* val, long long n_pairs, const int* ga, const int* gb, int skip, double* out) {
    HostChol& h = *static_cast<HostChol*>(p);
    const int nc = h.nc();
    std::vector<int64_t> gp(group_ptr, group_ptr + n_groups + 1), rp(row_ptr, row_ptr + group_ptr[n_groups] + 1);
    const pgo::ScRows R(h.N, h.in_system.data(), h.pos.data(), nc, n_groups, gp.data(), rp.data(), col, val);
    if (R.error) return -1;
    std::vector<double> W((size_t)R.rows * nc, 0.0), Y((size_t)R.rows * nc, 0.0), part((size_t)6 * pgo::DC_GRAM);
    for (size_t e = 0; e < R.at.size(); ++e) W[(size_t)R.at[e]] = R.val[e];
    const int k0 = skip ? R.first_tile : 0;
    for (int64_t r = 0; r < R.rows; ++r) {
        pgo::ScHost H{h.P, h.T.data(), W.data() + (size_t)r * nc, Y.data() + (size_t)r * nc, nullptr};
        for (int k = k0; k < h.P.nt; ++k) H.forward(k);
    }
    const int c0 = skip ? std::min(R.first_tile * pgo::DC_NB, nc) / pgo::DC_GRAM * pgo::DC_GRAM : 0;
    for (long long k = 0; k < n_pairs; ++k)
        pgo::dc_param_gram(pgo::DcSerial{}, Y.data() + (size_t)R.first_row[(size_t)ga[k]] * nc, R.dim[(size_t)ga[k]], Y.data() + (size_t)R.first_row[(size_t)gb[k]] * nc, R.dim[(size_t)gb[k]],
                           (size_t)nc, nc, c0, false, 0.0, part.data(), out + 36 * k);
    return 0;
}
}

#ifdef SPH_MAIN
#include <cstdio>

static double lcg(unsigned long long& s) { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return (double)((s >> 11) & ((1ULL << 53) - 1)) / (double)(1ULL << 53) - 0.5; }

int main() {
    int bad = 0;
    // a chain of 40 keyframes with two loop closures, keyframes 11 and 39 outside the system: diagonally dominant blocks
    const long long N = 40;
    std::vector<unsigned char> in((size_t)N, 1); in[11] = in[39] = 0;
    std::vector<int> hi, lo;
    for (int i = 0; i + 1 < N; ++i) if (in[(size_t)i] && in[(size_t)i + 1]) { hi.push_back(i % 2 ? i : i + 1); lo.push_back(i % 2 ? i + 1 : i); }      // (either of the two may be the higher)
    hi.push_back(37); lo.push_back(2); hi.push_back(10); lo.push_back(12);
    const long long np = (long long)hi.size();
    unsigned long long s = 5ULL;
    std::vector<double> diag((size_t)N * 36, 0.0), blocks((size_t)np * 36);
    for (double& v : blocks) v = lcg(s);
    for (long long i = 0; i < N; ++i) for (int a = 0; a < 6; ++a) for (int c = 0; c <= a; ++c) { const double v = a == c ? 30.0 + lcg(s) : lcg(s); diag[(size_t)i * 36 + a * 6 + c] = diag[(size_t)i * 36 + c * 6 + a] = v; }
    // the same matrix, dense, in the caller's order
    const int n = (int)N * 6;
    std::vector<double> A((size_t)n * n, 0.0);
    for (long long i = 0; i < N; ++i) for (int a = 0; a < 6; ++a) for (int c = 0; c < 6; ++c) A[(size_t)(i * 6 + a) * n + i * 6 + c] = in[(size_t)i] ? diag[(size_t)i * 36 + a * 6 + c] : (a == c ? 1.0 : 0.0);
    for (long long k = 0; k < np; ++k) for (int a = 0; a < 6; ++a) for (int c = 0; c < 6; ++c) A[(size_t)(hi[k] * 6 + a) * n + lo[k] * 6 + c] = A[(size_t)(lo[k] * 6 + c) * n + hi[k] * 6 + a] = blocks[(size_t)k * 36 + a * 6 + c];
    std::vector<double> B((size_t)2 * n), X((size_t)2 * n, 7.0);
    for (double& v : B) v = lcg(s);
    for (int ordering : {0, 1, -1}) {
        void* h = sph_create(N, in.data(), np, hi.data(), lo.data(), ordering);
        if (!h) { std::printf("ordering %d: the pairs were refused\n", ordering); ++bad; continue; }
        long long info[8]; std::vector<int> order((size_t)N);
        sph_info(h, info, order.data());
        if (!sph_factor(h, diag.data(), blocks.data())) { std::printf("ordering %d: reported not positive definite\n", ordering); ++bad; sph_destroy(h); continue; }
        sph_solve(h, 2, B.data(), X.data());
        double rmax = 0.0;
        for (int r = 0; r < 2; ++r)
            for (int i = 0; i < n; ++i) {
                if (!in[(size_t)i / 6]) { if (X[(size_t)r * n + i] != 0.0) { std::printf("ordering %d: an outside entry is not zero\n", ordering); ++bad; } continue; }
                double t = B[(size_t)r * n + i];
                for (int j = 0; j < n; ++j) t -= A[(size_t)i * n + j] * X[(size_t)r * n + j];
                rmax = std::fmax(rmax, std::fabs(t));
            }
        std::printf("ordering %d (used %lld): %lld tiles of L, residual %.3e\n", ordering, info[3], info[2], rmax);
        if (!(rmax <= 1e-12)) ++bad;
        // inverse blocks: keyframe 38 (six unit rows), keyframe 10, one two-keyframe row; (a, b) and (b, a) are exact transposes; against the solve
        std::vector<long long> gp = {0, 6, 12, 13}, rp = {0};
        std::vector<int> col; std::vector<double> val;
        for (int node : {38, 10}) for (int a = 0; a < 6; ++a) { col.push_back(node * 6 + a); val.push_back(1.0); rp.push_back((long long)col.size()); }
        for (int c : {12, 13, 14, 15, 16, 17, 222, 223, 224, 225, 226, 227}) { col.push_back(c); val.push_back(lcg(s)); }
        rp.push_back((long long)col.size());
        const int ga[5] = {0, 0, 1, 2, 2}, gb[5] = {0, 1, 0, 2, 0};
        std::vector<double> out((size_t)5 * 36, 7.0), out0(out);
        if (sph_inverse_blocks(h, 3, gp.data(), rp.data(), col.data(), val.data(), 5, ga, gb, 1, out.data()) != 0 || sph_inverse_blocks(h, 3, gp.data(), rp.data(), col.data(), val.data(), 5, ga, gb, 0, out0.data()) != 0) {
            std::printf("ordering %d: the rows were refused\n", ordering); ++bad;
        } else {
            if (std::memcmp(out.data(), out0.data(), out.size() * sizeof(double)) != 0) { std::printf("ordering %d: skipping the leading steps changed the bits\n", ordering); ++bad; }
            for (int a = 0; a < 6; ++a) for (int c = 0; c < 6; ++c) if (out[36 + a * 6 + c] != out[72 + c * 6 + a]) { std::printf("ordering %d: (b, a) is not the transpose of (a, b)\n", ordering); ++bad; a = c = 6; }
            std::vector<double> e((size_t)n, 0.0), col38((size_t)n);
            e[38 * 6 + 2] = 1.0;
            sph_solve(h, 1, e.data(), col38.data());
            double d = 0.0;
            for (int a = 0; a < 6; ++a) d = std::fmax(d, std::fabs(out[(size_t)a * 6 + 2] - col38[(size_t)38 * 6 + a]));
            if (!(d <= 1e-13)) { std::printf("ordering %d: the block of keyframe 38 is not the inverse's (%.3e)\n", ordering, d); ++bad; }
        }
        col[0] = 11 * 6;      // a row on a keyframe outside the system
        if (sph_inverse_blocks(h, 3, gp.data(), rp.data(), col.data(), val.data(), 5, ga, gb, 1, out.data()) == 0) { std::printf("a row outside the system was accepted\n"); ++bad; }
        sph_destroy(h);
    }
    {   // refused pair lists: a duplicate in the other order, an outside keyframe, a keyframe with itself
        std::vector<int> h2(hi), l2(lo);
        h2.push_back(lo[0]); l2.push_back(hi[0]);
        if (sph_create(N, in.data(), (long long)h2.size(), h2.data(), l2.data(), 0)) { std::printf("a duplicate pair was accepted\n"); ++bad; }
        h2.back() = 11; l2.back() = 3;
        if (sph_create(N, in.data(), (long long)h2.size(), h2.data(), l2.data(), 0)) { std::printf("a pair with an outside keyframe was accepted\n"); ++bad; }
        h2.back() = 5; l2.back() = 5;
        if (sph_create(N, in.data(), (long long)h2.size(), h2.data(), l2.data(), 0)) { std::printf("a keyframe paired with itself was accepted\n"); ++bad; }
    }
    {   // the reduction: 4 keyframes, keyframe 2 constant, parallel edges on (0, 1) in both orders
        const unsigned char fr[4] = {1, 1, 0, 1};
        const int rc1[3] = {0, 1, 2}, rc2[3] = {1, 0, 3}, sc1[2] = {3, 0}, sc2[2] = {0, 2};
        unsigned long long t = 99ULL;
        std::vector<double> hd((size_t)4 * 36), hoff((size_t)5 * 36), c((size_t)2 * 12), hh = {1.5, 2.5}, sd((size_t)4 * 36), sb((size_t)5 * 36);
        for (std::vector<double>* v : {&hd, &hoff, &c}) for (double& x : *v) x = lcg(t);
        int ph[5], pl[5];
        const long long m = sph_reduce(4, fr, hd.data(), hoff.data(), c.data(), hh.data(), 3, rc1, rc2, 2, sc1, sc2, ph, pl, sd.data(), sb.data());
        const double want = hoff[0 * 36 + 1 * 6 + 2] + hoff[1 * 36 + 2 * 6 + 1];      // block (1, 0), entry (2, 1): edge 0 transposed, edge 1 as it is
        if (m != 2 || ph[0] != 1 || pl[0] != 0 || ph[1] != 3 || pl[1] != 0 || sb[2 * 6 + 1] != want || sd[2 * 36] != 0.0) { std::printf("the reduction: wrong\n"); ++bad; }
    }
    std::printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}
#endif
