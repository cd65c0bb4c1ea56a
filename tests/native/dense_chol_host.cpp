// Host instantiation of the dense Cholesky solver's arithmetic (csrc/pgo_dense_math.hpp): the blocked factor and solve run serially, in the order of block steps and
// with the block routines the kernels of pgo_dense.hip use.  Built as a shared object for tests/test_dense_cholesky_host.py, or — with -DDCH_MAIN — as a stand-alone
// program that solves a few systems (orders with and without padding, an indefinite matrix, a NaN) and checks them itself: the form to run under
// -fsanitize=address,undefined.
#include "pgo_dense_math.hpp"

extern "C" {
// 1: solved; 0: a pivot was not positive (x untouched)
int dch_solve(int n, const double* a, const double* b, double* x) { return pgo::dc_host_solve(n, a, b, x) ? 1 : 0; }
// the 64 x 64 block routines on their own: factor of a (row-major 64 x 64, lower triangle read) into l (row-major, lower triangle + zeros), then L y = b, L^T x = y
int dch_block(const double* a, const double* b, double* l, double* y, double* x) {
    std::vector<double> blk((size_t)pgo::DC_NB * pgo::DC_LD, 0.0);
    for (int i = 0; i < pgo::DC_NB; ++i) for (int j = 0; j < pgo::DC_NB; ++j) blk[(size_t)i * pgo::DC_LD + j] = a[i * pgo::DC_NB + j];
    if (pgo::dc_factor_block(pgo::DcSerial{}, blk.data())) return 0;
    for (int i = 0; i < pgo::DC_NB; ++i) for (int j = 0; j < pgo::DC_NB; ++j) l[i * pgo::DC_NB + j] = j <= i ? blk[(size_t)i * pgo::DC_LD + j] : 0.0;
    double v[pgo::DC_NB];
    for (int i = 0; i < pgo::DC_NB; ++i) v[i] = b[i];
    pgo::dc_forward_block(pgo::DcSerial{}, blk.data(), v, y);
    for (int i = 0; i < pgo::DC_NB; ++i) v[i] = y[i];
    pgo::dc_backward_block(pgo::DcSerial{}, blk.data(), v, x);
    return 1;
}
}

#ifdef DCH_MAIN
#include <cstdio>
#include <limits>

static double lcg(unsigned long long& s) { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return (double)((s >> 11) & ((1ULL << 53) - 1)) / (double)(1ULL << 53) - 0.5; }

int main() {
    int bad = 0;
    for (int n : {64, 96, 200}) {
        unsigned long long s = 1234567ULL + (unsigned long long)n;
        const int m = n / 2 > 8 ? n / 2 : 8;
        std::vector<double> B((size_t)n * m), A((size_t)n * n, 0.0), b((size_t)n), x((size_t)n, 0.0);
        for (double& v : B) v = lcg(s);
        for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) { double t = 0.0; for (int k = 0; k < m; ++k) t += B[(size_t)i * m + k] * B[(size_t)j * m + k]; A[(size_t)i * n + j] = t; }
        for (int i = 0; i < n; ++i) { A[(size_t)i * n + i] += 1e-3 + 0.5 + lcg(s); b[i] = lcg(s); }
        if (!dch_solve(n, A.data(), b.data(), x.data())) { std::printf("n = %d: reported not positive definite\n", n); ++bad; continue; }
        double rmax = 0.0, anorm = 0.0, xmax = 0.0, bmax = 0.0;
        for (int i = 0; i < n; ++i) {
            double r = b[i], rowsum = 0.0;
            for (int j = 0; j < n; ++j) { r -= A[(size_t)i * n + j] * x[j]; rowsum += std::fabs(A[(size_t)i * n + j]); }
            rmax = std::fmax(rmax, std::fabs(r)); anorm = std::fmax(anorm, rowsum); xmax = std::fmax(xmax, std::fabs(x[i])); bmax = std::fmax(bmax, std::fabs(b[i]));
        }
        const double eta = rmax / (anorm * xmax + bmax), bound = 2.0 * n * std::numeric_limits<double>::epsilon() / 2.0;      // (n u for the solve + n u for this residual's own rounding)
        std::printf("n = %d: eta = %.3e (bound %.3e)\n", n, eta, bound);
        if (!(eta <= bound)) ++bad;
    }
    {
        std::vector<double> A((size_t)128 * 128, 0.0), b(128, 1.0), x(128, 7.0);
        for (int i = 0; i < 128; ++i) A[(size_t)i * 128 + i] = 1.0;
        A[(size_t)70 * 128 + 70] = -1.0;
        if (dch_solve(128, A.data(), b.data(), x.data()) || x[0] != 7.0) { std::printf("indefinite matrix: not reported\n"); ++bad; }
        A[(size_t)70 * 128 + 70] = 1.0;
        A[(size_t)100 * 128 + 3] = A[(size_t)3 * 128 + 100] = std::numeric_limits<double>::quiet_NaN();
        if (dch_solve(128, A.data(), b.data(), x.data())) { std::printf("NaN: not reported\n"); ++bad; }
    }
    std::printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}
#endif
