// Host instantiation of pgo_covariance's arithmetic (csrc/pgo_dense_math.hpp): the request plan with switch rows, the right-hand sides, the substitution in its block
// steps, the Gram products of 6- and 1-row blocks, and the matrix-free handle's matrix from its normal blocks — run serially with the routines the kernels of
// pgo_dense.hip call.  Built as a shared object for tests/test_param_cov_host.py, or — with -DMAIN — as a stand-alone program that checks itself (H Sigma = I on the full
// matrix with the switches, zero skipping, transposes, a refused h, a switch without a node): the form to run under -fsanitize=address,undefined.
#include "pgo_dense_math.hpp"

extern "C" {
// 1: computed; 0: a pivot was not positive or a requested switch's h cannot divide (cov untouched).  cov: n_pairs x 36
int pcv_covariance(int n, const double* a, const int* sw_node, const double* sw_c, const double* sw_h, long long n_pairs, const int* ia, const int* ib, int skip, double* cov) {
    return pgo::dc_host_param_covariance(n, a, sw_node, sw_c, sw_h, n_pairs, ia, ib, skip != 0, cov) ? 1 : 0;
}
// the request plan: returns m; col, first_col: room for 6 x (ids) + 64 entries; start_tile: m / 64
int pcv_plan(int n, int n_nodes, const int* sw_node, long long n_pairs, const int* ia, const int* ib, int* col, int* first_col, int* start_tile) {
    const pgo::DcParamPlan Q(n, n_nodes, sw_node, n_pairs, ia, ib);
    for (int r = 0; r < Q.m; ++r) { col[r] = Q.col[(size_t)r]; first_col[r] = Q.first_col[(size_t)r]; }
    for (int R = 0; R < Q.mt; ++R) start_tile[R] = Q.start_tile[(size_t)R];
    return Q.m;
}
// the matrix of a matrix-free handle from its normal blocks into the zeroed A (n x n, n >= 6 N a multiple of 64).  Returns the number of off-diagonal blocks written.
long long pcv_mf_matrix(long long N, const unsigned char* node_free, long long n_rel, const int* rc1, const int* rc2, long long n_sw, const int* sc1, const int* sc2,
                        const double* hd, const double* hoff, const double* sw_c, const double* sw_h, int n, double* A) {
    const pgo::DcMfPlan M(N, node_free, n_rel, rc1, rc2, n_sw, sc1, sc2);
    pgo::dc_host_mf_matrix(N, node_free, n_rel, M, hd, hoff, sw_c, sw_h, n, A);
    return M.segments();
}
}

#ifdef MAIN
#include <cstdio>
#include <cstring>

static double lcg(unsigned long long& s) { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return (double)((s >> 11) & ((1ULL << 53) - 1)) / (double)(1ULL << 53) - 0.5; }

int main() {
    int bad = 0;
    for (int n : {64, 66, 192}) {
        unsigned long long s = 1234567ULL + (unsigned long long)n;
        const int m = n / 2 > 8 ? n / 2 : 8, nodes = n / 6, ns = 7;
        std::vector<double> B((size_t)n * m), A((size_t)n * n, 0.0);
        for (double& v : B) v = lcg(s);
        for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) { double t = 0.0; for (int k = 0; k < m; ++k) t += B[(size_t)i * m + k] * B[(size_t)j * m + k]; A[(size_t)i * n + j] = t; }
        for (int i = 0; i < n; ++i) A[(size_t)i * n + i] += 1e-3 + 0.5 + lcg(s);
        // switch columns: both orders of the nodes, the first and the last node, one side dropped, no side at all
        std::vector<int> nd = {0, nodes - 1, nodes - 1, 0, 3, 2, 2, 3, 5, -1, -1, nodes - 2, -1, -1};
        std::vector<double> c((size_t)ns * 12), h((size_t)ns);
        for (double& v : c) v = 0.3 * lcg(s);
        for (double& v : h) v = 0.75 + lcg(s);
        const int ids = nodes + ns;
        std::vector<int> ia, ib;
        for (int a = 0; a < ids; ++a) for (int b = 0; b < ids; ++b) { ia.push_back(a); ib.push_back(b); }
        std::vector<double> c0(ia.size() * 36, 7.0), c1(ia.size() * 36, 7.0);
        if (!pcv_covariance(n, A.data(), nd.data(), c.data(), h.data(), (long long)ia.size(), ia.data(), ib.data(), 1, c0.data()) ||
            !pcv_covariance(n, A.data(), nd.data(), c.data(), h.data(), (long long)ia.size(), ia.data(), ib.data(), 0, c1.data())) { std::printf("n = %d: reported a failure\n", n); ++bad; continue; }
        if (std::memcmp(c0.data(), c1.data(), c0.size() * sizeof(double)) != 0) { std::printf("n = %d: zero skipping changed the bits\n", n); ++bad; }
        // Sigma over the 6 nodes + ns parameters, from the blocks
        const int np = 6 * nodes, nf = np + ns;
        auto dim = [&](int id) { return id < nodes ? 6 : 1; };
        auto off = [&](int id) { return id < nodes ? 6 * id : np + (id - nodes); };
        std::vector<double> Sg((size_t)nf * nf, 0.0);
        for (size_t k = 0; k < ia.size(); ++k) {
            const int da = dim(ia[k]), db = dim(ib[k]);
            for (int i = 0; i < da; ++i) for (int j = 0; j < db; ++j) Sg[(size_t)(off(ia[k]) + i) * nf + off(ib[k]) + j] = c0[k * 36 + (size_t)i * db + j];
            for (int e = da * db; e < 36; ++e) if (c0[k * 36 + e] != 0.0) { std::printf("n = %d: the rest of a block is not zero\n", n); ++bad; break; }
        }
        double asym = 0.0;
        for (int i = 0; i < nf; ++i) for (int j = 0; j < nf; ++j) asym = std::fmax(asym, std::fabs(Sg[(size_t)i * nf + j] - Sg[(size_t)j * nf + i]));
        if (asym != 0.0) { std::printf("n = %d: cov(b, a) is not the exact transpose of cov(a, b) (%.3e)\n", n, asym); ++bad; }
        if (Sg[(size_t)(np + 6) * nf + np + 6] != 1.0 / h[6]) { std::printf("n = %d: a switch without a node does not have variance 1 / h\n", n); ++bad; }
        if (np == n) {
            // H = [S + C diag(h)^-1 C^T, C; C^T, diag(h)]
            std::vector<double> H((size_t)nf * nf, 0.0);
            for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) H[(size_t)i * nf + j] = A[(size_t)i * n + j];
            for (int e = 0; e < ns; ++e) {
                std::vector<double> col((size_t)n, 0.0);
                for (int side = 0; side < 2; ++side) if (nd[2 * e + side] >= 0) for (int k = 0; k < 6; ++k) col[(size_t)nd[2 * e + side] * 6 + k] = c[(size_t)e * 12 + side * 6 + k];
                for (int i = 0; i < n; ++i) { H[(size_t)i * nf + np + e] = H[(size_t)(np + e) * nf + i] = col[i]; for (int j = 0; j < n; ++j) H[(size_t)i * nf + j] += col[i] * col[j] / h[e]; }
                H[(size_t)(np + e) * nf + np + e] = h[e];
            }
            double rmax = 0.0;
            for (int i = 0; i < nf; ++i) for (int j = 0; j < nf; ++j) { double t = i == j ? -1.0 : 0.0; for (int k = 0; k < nf; ++k) t += H[(size_t)i * nf + k] * Sg[(size_t)k * nf + j]; rmax = std::fmax(rmax, std::fabs(t)); }
            std::printf("n = %d + %d switches: |H Sigma - I|_max = %.3e\n", n, ns, rmax);
            if (!(rmax <= 1e-9)) ++bad;
        } else std::printf("n = %d: %d nodes + %d switches\n", n, nodes, ns);
        // a requested switch whose h cannot divide is refused, one nobody asked for is not looked at
        std::vector<double> hb(h); hb[1] = 0.0;
        const int a = nodes + 1, b = nodes + 2;
        std::vector<double> out(36, 7.0);
        if (pcv_covariance(n, A.data(), nd.data(), c.data(), hb.data(), 1, &a, &a, 1, out.data()) || out[0] != 7.0) { std::printf("n = %d: h = 0 not reported\n", n); ++bad; }
        if (!pcv_covariance(n, A.data(), nd.data(), c.data(), hb.data(), 1, &b, &b, 1, out.data())) { std::printf("n = %d: an unrequested switch's h was looked at\n", n); ++bad; }
    }
    {   // the matrix of a matrix-free handle: 4 keyframes, keyframe 2 constant, parallel edges on (0, 1) in both orders, every write inside n x n
        const int N = 4, n = 64;
        const unsigned char fr[4] = {1, 1, 0, 1};
        const int rc1[3] = {0, 1, 2}, rc2[3] = {1, 0, 3}, sc1[2] = {3, 0}, sc2[2] = {0, 2};
        unsigned long long s = 99ULL;
        std::vector<double> hd((size_t)N * 36), hoff((size_t)5 * 36), c((size_t)2 * 12), h = {1.5, 2.5}, A((size_t)n * n, 0.0);
        for (std::vector<double>* v : {&hd, &hoff, &c}) for (double& x : *v) x = lcg(s);
        const long long segs = pcv_mf_matrix(N, fr, 3, rc1, rc2, 2, sc1, sc2, hd.data(), hoff.data(), c.data(), h.data(), n, A.data());
        const double want = hoff[0 * 36 + 1 * 6 + 2] + hoff[1 * 36 + 2 * 6 + 1];      // block (1, 0), entry (2, 1): edge 0 transposed (its c1 is the lower keyframe), edge 1 as it is
        if (segs != 2 || A[(size_t)(6 + 2) * n + 1] != want || A[(size_t)14 * n + 14] != 1.0 || A[(size_t)63 * n + 63] != 1.0 || A[(size_t)1 * n + 8] != 0.0) { std::printf("matrix-free matrix: wrong\n"); ++bad; }
    }
    std::printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}
#endif
