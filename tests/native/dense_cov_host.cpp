// Host instantiation of the covariance blocks' arithmetic (csrc/pgo_dense_math.hpp): the blocked factor, the forward substitution with many right-hand sides and the Gram
// products run serially, in the order of block steps and with the block routines the kernels of pgo_dense.hip use.  Built as a shared object for
// tests/test_dense_cov_host.py, or — with -DDCV_MAIN — as a stand-alone program that computes a few blocks (orders with and without padding, zero skipping on and off, an
// indefinite matrix) and checks them itself: the form to run under -fsanitize=address,undefined.
#include "pgo_dense_math.hpp"

extern "C" {
// 1: computed; 0: a pivot was not positive (cov untouched).  cov: n_pairs x 36.  Node blocks only (0 <= ia, ib < n / 6): a request without switches
int dcv_covariance(int n, const double* a, long long n_pairs, const int* ia, const int* ib, int skip, double* cov) {
    return pgo::dc_host_param_covariance(n, a, nullptr, nullptr, nullptr, n_pairs, ia, ib, skip != 0, cov) ? 1 : 0;
}
}

#ifdef DCV_MAIN
#include <cstdio>
#include <cstring>

static double lcg(unsigned long long& s) { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return (double)((s >> 11) & ((1ULL << 53) - 1)) / (double)(1ULL << 53) - 0.5; }

int main() {
    int bad = 0;
    for (int n : {64, 66, 192}) {
        unsigned long long s = 7654321ULL + (unsigned long long)n;
        const int m = n / 2 > 8 ? n / 2 : 8, last = n / 6 - 1;
        std::vector<double> B((size_t)n * m), A((size_t)n * n, 0.0);
        for (double& v : B) v = lcg(s);
        for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) { double t = 0.0; for (int k = 0; k < m; ++k) t += B[(size_t)i * m + k] * B[(size_t)j * m + k]; A[(size_t)i * n + j] = t; }
        for (int i = 0; i < n; ++i) A[(size_t)i * n + i] += 1e-3 + 0.5 + lcg(s);
        // every node once, so that the blocks are whole block columns of the inverse: A Sigma = I can be checked
        std::vector<int> ia, ib;
        for (int a = 0; a <= last; ++a) for (int b = 0; b <= last; ++b) { ia.push_back(a); ib.push_back(b); }
        std::vector<double> c0(ia.size() * 36, 7.0), c1(ia.size() * 36, 7.0);
        if (!dcv_covariance(n, A.data(), (long long)ia.size(), ia.data(), ib.data(), 1, c0.data()) || !dcv_covariance(n, A.data(), (long long)ia.size(), ia.data(), ib.data(), 0, c1.data())) {
            std::printf("n = %d: reported not positive definite\n", n); ++bad; continue;
        }
        if (std::memcmp(c0.data(), c1.data(), c0.size() * sizeof(double)) != 0) { std::printf("n = %d: zero skipping changed the bits\n", n); ++bad; }
        const int nn = 6 * (last + 1);      // the leading nn x nn part of the inverse; the rows of A beyond it (n = 64: 60-63, n = 66: none, n = 192: none) couple to it
        auto sig = [&](int i, int j) { return c0[((size_t)(i / 6) * (last + 1) + j / 6) * 36 + (i % 6) * 6 + j % 6]; };
        double asym = 0.0;
        for (int i = 0; i < nn; ++i) for (int j = 0; j < nn; ++j) asym = std::fmax(asym, std::fabs(sig(i, j) - sig(j, i)));
        if (asym != 0.0) { std::printf("n = %d: cov(b, a) is not the exact transpose of cov(a, b) (%.3e)\n", n, asym); ++bad; }
        if (nn == n) {
            double rmax = 0.0;
            for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) { double t = i == j ? -1.0 : 0.0; for (int k = 0; k < n; ++k) t += A[(size_t)i * n + k] * sig(k, j); rmax = std::fmax(rmax, std::fabs(t)); }
            std::printf("n = %d: |A Sigma - I|_max = %.3e\n", n, rmax);
            if (!(rmax <= 1e-9)) ++bad;
        } else std::printf("n = %d: %d nodes\n", n, last + 1);
    }
    {
        std::vector<double> A((size_t)128 * 128, 0.0), c(36, 7.0);
        for (int i = 0; i < 128; ++i) A[(size_t)i * 128 + i] = 1.0;
        A[(size_t)70 * 128 + 70] = -1.0;
        const int a = 3;
        if (dcv_covariance(128, A.data(), 1, &a, &a, 1, c.data()) || c[0] != 7.0) { std::printf("indefinite matrix: not reported\n"); ++bad; }
    }
    std::printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}
#endif
