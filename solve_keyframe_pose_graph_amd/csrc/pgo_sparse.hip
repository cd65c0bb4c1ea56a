// pgo_sparse.hip — libpgo_sparse.so (include/pgo_sparse.h): the tile-sparse exact Cholesky solver on the device.  The six kernels of pgo_dense.hip with the matrix
// addressed through an ScPlan (pgo_sparse_math.hpp): tile storage `tiles` x 4096 doubles, the plan's tables on the device as int32.  The arithmetic of the diagonal
// tile, the panel, the update and the two sweeps is COPIED from dc_first_block_kernel, dc_panel_kernel, dc_update_kernel, dc_forward_kernel and dc_backward_kernel —
// the same MFMA operand maps (the comment above dc_panel_kernel), the same summation order, the block routines of pgo_dense_math.hpp — on purpose: the originals live in
// an anonymous namespace of a translation unit of libpgo.so, which this library neither links nor changes.  In natural order the results are the dense solver's as numbers.
//
// Nothing waits on another workgroup inside a launch, there are no atomics, every sum has a fixed order.  The step order is sc_factor_steps / sc_solve_steps, nowhere
// else.  The update finds its target tile by ScPlan::find's binary search in row_col, in device code (sc_find): no per-step pair table.
//
// The selected inverse (sc_selinv_steps: sc_sel_inverses_kernel, sc_sel_ginv_kernel, sc_sel_column_kernel, sc_sel_diag_kernel, then sc_sel_gather_kernel for 6 x 6 blocks)
// has no counterpart in pgo_dense.hip: Takahashi's recurrence on the tiles of L into a second tile array, under the same rules.
//
// The columns of the inverse in number (sc_panel_steps: sc_pcol_rhs_kernel, sc_pfwd_kernel, sc_pbwd_kernel, sc_pgather_kernel) are the tile-sparse counterpart of
// dcv_solve_kernel / dcv_update_kernel — right-hand sides as the rows of W, 64 per workgroup — in the pull form and for both sweeps: blocks outside the pattern of L.
//
// The exact LM step and solve on this factor (pgo_sparse_lm_*: sc_lm_scale_kernel, sc_lm_fill_kernel, sc_lm_rhs_kernel, sc_lm_backsub_kernel, sc_lm_model_kernel,
// sc_lm_reduce_kernel) are in pgo_sparse_lm.hpp, included at the end of this file: still one translation unit.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>

#include "pgo_sparse.h"
#include "pgo_sparse_blocks.hpp"

namespace pgo {

namespace {

typedef double sc_d4 __attribute__((ext_vector_type(4)));
constexpr int SC_THREADS = 256;

struct ScTeam {
    __device__ __forceinline__ int rank() const { return (int)threadIdx.x; }
    __device__ __forceinline__ int size() const { return SC_THREADS; }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
};

// the plan's tables on the device
struct ScDev { const int32_t* row_ptr; const int32_t* row_col; const int32_t* col_ptr; const int32_t* col_row; const int32_t* col_tile; const int32_t* ahead; };

// ScPlan::find: the id of tile (i, j), j <= i; -1: not in the pattern
__device__ __forceinline__ int sc_find(const ScDev& P, int i, int j) {
    int lo = P.row_ptr[i];
    const int end = P.row_ptr[i + 1];
    int hi = end;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (P.row_col[mid] < j) lo = mid + 1; else hi = mid; }
    return lo < end && P.row_col[lo] == j ? lo : -1;
}

// a stored tile -> LDS, all of it (the part above the diagonal of a diagonal tile is never read)
__device__ __forceinline__ void sc_load_tile(const double* __restrict__ t, double* __restrict__ l) {
    for (int idx = threadIdx.x; idx < DC_NB * DC_NB; idx += SC_THREADS) l[(idx >> 6) * DC_LD + (idx & 63)] = t[idx];
}
// the factored tile's lower triangle -> its storage
__device__ __forceinline__ void sc_store_lower(double* __restrict__ t, const double* __restrict__ l) {
    for (int idx = threadIdx.x; idx < DC_NB * DC_NB; idx += SC_THREADS) {
        const int r = idx >> 6, c = idx & 63;
        if (c <= r) t[idx] = l[r * DC_LD + c];
    }
}

// diag: the diagonal tile of step 0, and every later one that no update factors one step ahead (an empty s_k, or k + 1 not in s_k)
__global__ __launch_bounds__(SC_THREADS) void sc_diag_kernel(double* __restrict__ T, int tile, int32_t* __restrict__ fail) {
    __shared__ double l[DC_NB * DC_LD];
    double* __restrict__ t = T + (size_t)tile * SC_TILE;
    sc_load_tile(t, l);
    __syncthreads();
    const bool bad = dc_factor_block(ScTeam{}, l);
    sc_store_lower(t, l);
    if (threadIdx.x == 0 && bad) *fail = 1;
}

// panel(k): one workgroup per tile of s_k (dc_panel_kernel's substitution, one wavefront per 16 rows).  Writes L_ik in place and, k-major, into LT[64][ldu] at the
// columns 64 e .. 64 e + 63 of the tile's POSITION e in s_k: the scratch is as wide as the longest s_k, not as the matrix.
__global__ __launch_bounds__(SC_THREADS) void sc_panel_kernel(double* __restrict__ T, ScDev P, int k, int ldu, double* __restrict__ LT) {
    __shared__ double l[DC_NB * DC_LD];
    sc_load_tile(T + (size_t)(P.row_ptr[k + 1] - 1) * SC_TILE, l);
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lr = lane & 15, lk = lane >> 4;
    const int e = (int)blockIdx.x;                                         // < |s_k|: the grid
    const int x0 = e * DC_NB + wave * DC_SUB;
    double* __restrict__ arow = T + (size_t)P.col_tile[P.col_ptr[k] + e] * SC_TILE + (size_t)(wave * DC_SUB + lr) * DC_NB;
    sc_d4 Y[DC_NB / DC_SUB];
#pragma unroll
    for (int j = 0; j < DC_NB / DC_SUB; ++j) {
        double r[4];
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) r[reg] = arow[j * DC_SUB + lk + 4 * reg];
        sc_d4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int m = 0; m < j; ++m)
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(l[(j * DC_SUB + lr) * DC_LD + m * DC_SUB + 4 * kk + lk], Y[m][kk], acc, 0, 0, 0);
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) r[reg] = r[reg] - acc[reg];
#pragma unroll
        for (int p = 0; p < DC_SUB; ++p) {
            const double yp = __shfl(r[p >> 2], (p & 3) * 16 + lr) / l[(j * DC_SUB + p) * DC_LD + j * DC_SUB + p];
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int q = lk + 4 * reg;
                const double lqp = l[(j * DC_SUB + (q > p ? q : p)) * DC_LD + j * DC_SUB + p];      // (q <= p: the diagonal entry, unused)
                r[reg] = q == p ? yp : (q > p ? r[reg] - lqp * yp : r[reg]);
            }
        }
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            Y[j][reg] = r[reg];
            arow[j * DC_SUB + lk + 4 * reg] = r[reg];
            LT[(size_t)(j * DC_SUB + lk + 4 * reg) * ldu + x0 + lr] = r[reg];
        }
    }
}

// update(k): one workgroup per pair a >= b of positions in s_k, decoded from the 1-D block index p = a (a + 1) / 2 + b; the tile (s_k[a], s_k[b]) -= L_a L_b^T as
// dc_update_kernel computes it, operands from the k-major copy.  Pair (0, 0) is tile (k + 1, k + 1) when ahead[k]: that workgroup keeps the tile in LDS and factors it.
__global__ __launch_bounds__(SC_THREADS) void sc_update_kernel(double* __restrict__ T, ScDev P, int k, int ldu, const double* __restrict__ LT, int32_t* __restrict__ fail) {
    __shared__ double a[DC_NB * DC_LD];
    const int p = (int)blockIdx.x;                                         // < |s_k| (|s_k| + 1) / 2: the grid
    int pa = (int)((sqrt(8.0 * (double)p + 1.0) - 1.0) * 0.5);
    while (pa * (pa + 1) / 2 > p) --pa;
    while ((pa + 1) * (pa + 2) / 2 <= p) ++pa;
    const int pb = p - pa * (pa + 1) / 2;
    const int c0 = P.col_ptr[k];
    const int id = sc_find(P, P.col_row[c0 + pa], P.col_row[c0 + pb]);      // in the pattern by construction of the symbolic factorisation
    if (id < 0) return;
    double* __restrict__ t = T + (size_t)id * SC_TILE;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lr = lane & 15, lk = lane >> 4;
    const int wr = wave >> 1, wc = wave & 1;
    const int i0 = wr * 32, j0 = wc * 32;                                  // inside the tile
    const int ia = pa * DC_NB + i0, jb = pb * DC_NB + j0;                  // columns of the k-major copy
    const bool ahead = p == 0 && P.ahead[k] != 0;                          // this workgroup owns the next diagonal tile
    if (!(pa == pb && wr == 0 && wc == 1)) {                               // (that quadrant lies above the diagonal)
        sc_d4 acc[2][2];
        double old[2][2][4];
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                acc[s][u] = sc_d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) old[s][u][reg] = t[(i0 + s * 16 + lk + 4 * reg) * DC_NB + j0 + u * 16 + lr];
            }
#pragma unroll
        for (int kk = 0; kk < DC_NB / 4; ++kk) {
            const size_t row = (size_t)(kk * 4 + lk) * ldu;
            const double a0 = LT[row + ia + lr], a1 = LT[row + ia + 16 + lr], b0 = LT[row + jb + lr], b1 = LT[row + jb + 16 + lr];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int i = i0 + s * 16 + lk + 4 * reg, j = j0 + u * 16 + lr;
                    const double v = old[s][u][reg] - acc[s][u][reg];
                    if (ahead) a[i * DC_LD + j] = v;      // (written to the tile once, as the factor)
                    else t[i * DC_NB + j] = v;
                }
    }
    if (!ahead) return;
    __syncthreads();
    const bool bad = dc_factor_block(ScTeam{}, a);
    sc_store_lower(t, a);
    if (threadIdx.x == 0 && bad) *fail = 1;
}

// forward(k), grid (1 + |s_k|, n_rhs): every workgroup solves L_kk y_k = w_k of its right-hand side in LDS; the first writes y_k, the one of position e takes
// L_ik y_k off the 64 rows i = s_k[e] of w
__global__ __launch_bounds__(SC_THREADS) void sc_forward_kernel(const double* __restrict__ T, ScDev P, int k, int nc, double* __restrict__ W, double* __restrict__ Yv) {
    __shared__ double l[DC_NB * DC_LD];
    __shared__ double v[DC_NB], y[DC_NB], part[DC_NB * 4];
    const int k0 = k * DC_NB, tid = threadIdx.x;
    double* __restrict__ w = W + (size_t)blockIdx.y * nc;
    double* __restrict__ yv = Yv + (size_t)blockIdx.y * nc;
    sc_load_tile(T + (size_t)(P.row_ptr[k + 1] - 1) * SC_TILE, l);
    if (tid < DC_NB) v[tid] = w[k0 + tid];
    __syncthreads();
    dc_forward_block(ScTeam{}, l, v, y);
    if (blockIdx.x == 0) { if (tid < DC_NB) yv[k0 + tid] = y[tid]; return; }
    const int e = P.col_ptr[k] + (int)blockIdx.x - 1;
    const int i0 = P.col_row[e] * DC_NB;
    const int r = tid >> 2, q = tid & 3;
    const double* __restrict__ arow = T + (size_t)P.col_tile[e] * SC_TILE + (size_t)r * DC_NB;
    double s = 0.0;
#pragma unroll
    for (int c = 16 * q; c < 16 * q + 16; ++c) s += arow[c] * y[c];
    part[r * 4 + q] = s;
    __syncthreads();
    if (tid < DC_NB) w[i0 + tid] -= dc_sum4(part[tid * 4], part[tid * 4 + 1], part[tid * 4 + 2], part[tid * 4 + 3]);
}

// backward(k), grid (tiles of tile row k, n_rhs): every workgroup solves L_kk^T x_k = y_k; the one of the diagonal tile writes x_k, the one of tile (k, j) takes
// L_kj^T x_k off the 64 entries j of y
__global__ __launch_bounds__(SC_THREADS) void sc_backward_kernel(const double* __restrict__ T, ScDev P, int k, int nc, double* __restrict__ Yv, double* __restrict__ X) {
    __shared__ double l[DC_NB * DC_LD];
    __shared__ double v[DC_NB], xs[DC_NB], part[DC_NB * 4];
    const int k0 = k * DC_NB, tid = threadIdx.x;
    double* __restrict__ yv = Yv + (size_t)blockIdx.y * nc;
    const int diag = P.row_ptr[k + 1] - 1, id = P.row_ptr[k] + (int)blockIdx.x;      // <= diag: the grid
    sc_load_tile(T + (size_t)diag * SC_TILE, l);
    if (tid < DC_NB) v[tid] = yv[k0 + tid];
    __syncthreads();
    dc_backward_block(ScTeam{}, l, v, xs);
    if (id == diag) { if (tid < DC_NB) X[(size_t)blockIdx.y * nc + k0 + tid] = xs[tid]; return; }
    const int j0 = P.row_col[id] * DC_NB;
    const double* __restrict__ t = T + (size_t)id * SC_TILE;
    const int c = tid & 63, q = tid >> 6;
    double s = 0.0;
#pragma unroll
    for (int r = 16 * q; r < 16 * q + 16; ++r) s += t[r * DC_NB + c] * xs[r];
    part[c * 4 + q] = s;
    __syncthreads();
    if (tid < DC_NB) yv[j0 + tid] -= dc_sum4(part[tid * 4], part[tid * 4 + 1], part[tid * 4 + 2], part[tid * 4 + 3]);
}

// fill: the caller's blocks into the zeroed tiles under the permutation (sc_block_entry), ones on the diagonal of the rows outside the system and of the padding.  One
// thread per entry: 36 per keyframe, the padding, 36 per pair.  Pure copies, one writer per address.
__global__ __launch_bounds__(SC_THREADS) void sc_fill_kernel(double* __restrict__ T, ScDev P, int64_t N, int nc, const uint8_t* __restrict__ in_system, const int32_t* __restrict__ pos,
                                                             const double* __restrict__ diag, int64_t n_pairs, const int32_t* __restrict__ hi, const int32_t* __restrict__ lo, const double* __restrict__ blocks) {
    const int64_t gid = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x;
    const int64_t n36 = N * 36, pad = (int64_t)nc - N * 6;
    int row, col;
    double v;
    if (gid < n36) {
        const int64_t node = gid / 36;
        const int e = (int)(gid - node * 36), a = e / 6, c = e - a * 6;
        if (!sc_block_entry(pos[node], pos[node], a, c, &row, &col)) return;
        if (in_system[node]) v = diag[gid];
        else if (a == c) v = 1.0;
        else return;
    } else if (gid < n36 + pad) {
        row = col = (int)(N * 6 + (gid - n36));
        v = 1.0;
    } else {
        const int64_t u = gid - n36 - pad, k = u / 36;
        if (k >= n_pairs) return;
        const int e = (int)(u - k * 36), a = e / 6, c = e - a * 6;
        sc_block_entry(pos[hi[k]], pos[lo[k]], a, c, &row, &col);
        v = blocks[u];
    }
    const int id = sc_find(P, row / DC_NB, col / DC_NB);
    if (id < 0) return;                                                    // (the pattern was made from these very pairs)
    T[(size_t)id * SC_TILE + (size_t)(row % DC_NB) * DC_NB + col % DC_NB] = v;
}

// the right-hand sides of the inverse blocks: every non-zero of P v into the zeroed W (the host checked that no two meet)
__global__ __launch_bounds__(SC_THREADS) void sc_rhs_kernel(double* __restrict__ W, int64_t nnz, const int64_t* __restrict__ at, const double* __restrict__ val) {
    const int64_t gid = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x;
    if (gid < nnz) W[at[gid]] = val[gid];
}

// gram: one workgroup per requested pair, pr[3 pair ..]: the first rows of Y of the two groups and their sizes (d_a | d_b << 8); dc_param_gram_block over the columns from c0 on
__global__ __launch_bounds__(SC_THREADS) void sc_gram_kernel(const double* __restrict__ Y, int nc, int c0, const int32_t* __restrict__ pr, double* __restrict__ out) {
    __shared__ double part[6 * DC_GRAM];
    const size_t pair = blockIdx.x;
    const int32_t* q = pr + 3 * pair;
    dc_param_gram(ScTeam{}, Y + (size_t)q[0] * nc, q[2] & 255, Y + (size_t)q[1] * nc, q[2] >> 8, (size_t)nc, nc, c0, false, 0.0, part, out + 36 * pair);
}

// ---- the selected inverse (sc_selinv_steps): Z, a second tile array with the ids of L's tiles; T is only read.  G: the tiles G_e = L_{s[e],k} L_kk^-1 of one step,
// row-major, compact by position e in s_k — the major order both column(k) (B operand: rows of G) and diag(k) (A operand: G^T) read with consecutive lanes.

// ginv(k): one workgroup per tile of s_k.  g L_kk = l per row, one wavefront per 16 rows: sc_panel_kernel's scheme run backwards — the 16-wide block columns from the
// last to the first, MFMA products with the block columns already solved (m = 3 .. j + 1), substitution inside the diagonal sub-block from its last column to its first.
// Operand map: A[i][k] = L[16 m + k][16 j + i], B[k][n] = G[row n][16 m + k], D[i][n] = (G_m L_mj)[row n][16 j + i]; a lane holds row lr, columns lk + 4 reg.
__global__ __launch_bounds__(SC_THREADS) void sc_sel_ginv_kernel(const double* __restrict__ T, ScDev P, int k, double* __restrict__ G) {
    __shared__ double l[DC_NB * DC_LD];
    sc_load_tile(T + (size_t)(P.row_ptr[k + 1] - 1) * SC_TILE, l);
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lr = lane & 15, lk = lane >> 4;
    const int e = (int)blockIdx.x;                                         // < |s_k|: the grid
    const double* __restrict__ arow = T + (size_t)P.col_tile[P.col_ptr[k] + e] * SC_TILE + (size_t)(wave * DC_SUB + lr) * DC_NB;
    double* __restrict__ grow = G + (size_t)e * SC_TILE + (size_t)(wave * DC_SUB + lr) * DC_NB;
    sc_d4 Y[DC_NB / DC_SUB];
#pragma unroll
    for (int j = DC_NB / DC_SUB - 1; j >= 0; --j) {
        double r[4];
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) r[reg] = arow[j * DC_SUB + lk + 4 * reg];
        sc_d4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int m = DC_NB / DC_SUB - 1; m > j; --m)
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(l[(m * DC_SUB + 4 * kk + lk) * DC_LD + j * DC_SUB + lr], Y[m][kk], acc, 0, 0, 0);
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) r[reg] = r[reg] - acc[reg];
#pragma unroll
        for (int p = DC_SUB - 1; p >= 0; --p) {
            const double gp = __shfl(r[p >> 2], (p & 3) * 16 + lr) / l[(j * DC_SUB + p) * DC_LD + j * DC_SUB + p];
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int q = lk + 4 * reg;
                const double lpq = l[(j * DC_SUB + p) * DC_LD + j * DC_SUB + (q < p ? q : p)];      // (q >= p: the diagonal entry, unused)
                r[reg] = q == p ? gp : (q < p ? r[reg] - lpq * gp : r[reg]);
            }
        }
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            Y[j][reg] = r[reg];
            grow[j * DC_SUB + lk + 4 * reg] = r[reg];
        }
    }
}

// column(k): one workgroup per position a; Z_{s[a],k} = - sum_b Z(s[a], s[b]) G_b.  2 x 2 MFMA tiles per wavefront over K = 64 (sc_update_kernel's layout), the
// accumulators carried in registers over b ascending.  The tile Z(s[a], s[b]) goes through LDS: stored as (s[a], s[b]) where a >= b, as (s[b], s[a]) — read transposed —
// where a < b; the stride of 65 makes both walks conflict-free.
__global__ __launch_bounds__(SC_THREADS) void sc_sel_column_kernel(double* __restrict__ Z, ScDev P, int k, const double* __restrict__ G) {
    __shared__ double z[DC_NB * DC_LD];
    const int a = (int)blockIdx.x;                                         // < |s_k|: the grid
    const int c0 = P.col_ptr[k], m = P.col_ptr[k + 1] - c0, ra = P.col_row[c0 + a];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lr = lane & 15, lk = lane >> 4;
    const int i0 = (wave >> 1) * 32, j0 = (wave & 1) * 32;                 // inside the tile
    sc_d4 acc[2][2];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int u = 0; u < 2; ++u) acc[s][u] = sc_d4{0.0, 0.0, 0.0, 0.0};
    for (int b = 0; b < m; ++b) {
        const int rb = P.col_row[c0 + b];
        const bool tr = a < b;
        const int id = tr ? sc_find(P, rb, ra) : sc_find(P, ra, rb);      // in the pattern by construction of the symbolic factorisation
        if (id < 0) return;                                                // (the same for every thread of the workgroup)
        __syncthreads();                                                   // the products of the tile before are done with z
        sc_load_tile(Z + (size_t)id * SC_TILE, z);
        __syncthreads();
        const int si = tr ? 1 : DC_LD, sk = tr ? DC_LD : 1;
        const double* __restrict__ g = G + (size_t)b * SC_TILE;
#pragma unroll
        for (int kk = 0; kk < DC_NB / 4; ++kk) {
            const int kx = kk * 4 + lk;
            const double a0 = z[(i0 + lr) * si + kx * sk], a1 = z[(i0 + 16 + lr) * si + kx * sk], b0 = g[kx * DC_NB + j0 + lr], b1 = g[kx * DC_NB + j0 + 16 + lr];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
    double* __restrict__ t = Z + (size_t)P.col_tile[c0 + a] * SC_TILE;      // a tile of column k: none of those read above
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) t[(i0 + s * 16 + lk + 4 * reg) * DC_NB + j0 + u * 16 + lr] = -acc[s][u][reg];
}

// inverses: one workgroup per diagonal tile k (the grid: nt), Z_kk = L_kk^-T L_kk^-1 in LDS from the 64 unit right-hand sides, thread c substituting column c in place
// (dc_forward_block, dc_backward_block); the entries i >= j, stored mirrored.  It reads L alone: one launch ahead of the chain of dependent steps.
__global__ __launch_bounds__(SC_THREADS) void sc_sel_inverses_kernel(const double* __restrict__ T, double* __restrict__ Z, ScDev P) {
    __shared__ double l[DC_NB * DC_LD];
    __shared__ double x[DC_NB * DC_LD];
    const int diag = P.row_ptr[blockIdx.x + 1] - 1;
    sc_load_tile(T + (size_t)diag * SC_TILE, l);
    for (int idx = threadIdx.x; idx < DC_NB * DC_NB; idx += SC_THREADS) x[(idx >> 6) * DC_LD + (idx & 63)] = (idx >> 6) == (idx & 63) ? 1.0 : 0.0;
    __syncthreads();
    if (threadIdx.x < DC_NB) {
        double* v = x + threadIdx.x * DC_LD;                               // column c of the inverse, entry p at v[p]
        dc_forward_block(DcSerial{}, l, v, v);
        dc_backward_block(DcSerial{}, l, v, v);
    }
    __syncthreads();
    double* __restrict__ t = Z + (size_t)diag * SC_TILE;
    for (int idx = threadIdx.x; idx < DC_NB * DC_NB; idx += SC_THREADS) {
        const int r = idx >> 6, c = idx & 63;
        t[idx] = c <= r ? x[c * DC_LD + r] : x[r * DC_LD + c];              // entry (i, j), i >= j: entry i of column j
    }
}

// diag(k): one workgroup.  Z_kk -= sum_a G_a^T Z_{s[a],k}, a ascending, 2 x 2 MFMA tiles per wavefront in the three quadrants on or below the diagonal; the entries
// i >= j, each written to both triangles by the one lane that holds it.
__global__ __launch_bounds__(SC_THREADS) void sc_sel_diag_kernel(double* __restrict__ Z, ScDev P, int k, const double* __restrict__ G) {
    const int c0 = P.col_ptr[k], m = P.col_ptr[k + 1] - c0;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lr = lane & 15, lk = lane >> 4;
    const int i0 = (wave >> 1) * 32, j0 = (wave & 1) * 32;
    if (i0 == 0 && j0 == 32) return;                                       // (that quadrant lies above the diagonal)
    sc_d4 acc[2][2];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int u = 0; u < 2; ++u) acc[s][u] = sc_d4{0.0, 0.0, 0.0, 0.0};
    for (int a = 0; a < m; ++a) {
        const double* __restrict__ g = G + (size_t)a * SC_TILE;
        const double* __restrict__ zt = Z + (size_t)P.col_tile[c0 + a] * SC_TILE;
#pragma unroll
        for (int kk = 0; kk < DC_NB / 4; ++kk) {
            const int kx = (kk * 4 + lk) * DC_NB;
            const double a0 = g[kx + i0 + lr], a1 = g[kx + i0 + 16 + lr], b0 = zt[kx + j0 + lr], b1 = zt[kx + j0 + 16 + lr];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
    double* t = Z + (size_t)(P.row_ptr[k + 1] - 1) * SC_TILE;              // the diagonal tile: none of those read above
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int i = i0 + s * 16 + lk + 4 * reg, j = j0 + u * 16 + lr;
                if (i >= j) {
                    const double v = t[i * DC_NB + j] - acc[s][u][reg];
                    t[i * DC_NB + j] = v;
                    t[j * DC_NB + i] = v;
                }
            }
}

// gather: one thread per entry of a requested 6 x 6 block of the inverse, rows of keyframe na, columns of keyframe nb in the caller's order (sc_selected_block_host).
// flag[block]: 1, or 0 where one of the (up to four) tiles the block touches is not in the pattern — that block comes back zero, not guessed.
__global__ __launch_bounds__(SC_THREADS) void sc_sel_gather_kernel(const double* __restrict__ Z, ScDev P, int64_t n_blocks, const int32_t* __restrict__ na, const int32_t* __restrict__ nb,
                                                                   const uint8_t* __restrict__ in_system, const int32_t* __restrict__ pos, double* __restrict__ out, uint8_t* __restrict__ flag) {
    const int64_t gid = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x, blk = gid / 36;
    if (blk >= n_blocks) return;
    const int e = (int)(gid - blk * 36), i = e / 6, j = e - i * 6;
    const int32_t a = na[blk], b = nb[blk];                                // both in 0 .. N - 1: the host checked
    bool in = true, zero = !in_system[a] || !in_system[b];
    int row, col;
    if (!zero) {
        for (int ci = 0; ci < 6; ci += 5)
            for (int cj = 0; cj < 6; cj += 5) { sc_sigma_entry(pos[a], pos[b], ci, cj, &row, &col); if (sc_find(P, row / DC_NB, col / DC_NB) < 0) in = false; }
    }
    if (e == 0) flag[blk] = in ? 1 : 0;
    double v = 0.0;
    if (!zero && in) {
        sc_sigma_entry(pos[a], pos[b], i, j, &row, &col);
        v = Z[(size_t)sc_find(P, row / DC_NB, col / DC_NB) * SC_TILE + (size_t)(row % DC_NB) * DC_NB + col % DC_NB];
    }
    out[gid] = v;
}

// ---- columns of the inverse in number (sc_panel_steps): W [m_pad][nc], the right-hand sides as rows, a workgroup per panel of 64 rows, a wavefront per 16 of them.
// A lane (lr, lk) holds row 16 wave + lr of the panel and the columns 16 jb + lk + 4 reg of the block W_pk — sc_panel_kernel's layout, so the product sums feed the
// substitution without a transposition.  For that the products are formed transposed, D^T = L W^T: the tile of L is the A operand (A[i][k], i the column of W_pk),
// the rows of W the B operand (B[k][n], n the row), and D comes back as col = lane & 15 = the row of W, row = (lane >> 4) + 4 reg = the column inside the 16-wide
// block.  The tile of L goes through LDS (all four wavefronts read all of it; the stride of 65 makes the row walk of the forward sweep and the column walk of the
// backward sweep conflict-free) and the diagonal tile follows it into the same 33 KB.  The rows of W are read directly, not through LDS: a wavefront reads its own 16
// rows and nobody else's, four consecutive doubles of each per load — staging them would take a second 33 KB array and the kernel past 64 KB of LDS per workgroup.

// rhs: the one of every unit row into the zeroed W; col[r] = -1: a padding row
__global__ __launch_bounds__(SC_THREADS) void sc_pcol_rhs_kernel(double* __restrict__ W, int nc, int rows, const int32_t* __restrict__ col) {
    const int r = (int)(blockIdx.x * SC_THREADS + threadIdx.x);
    if (r < rows && col[r] >= 0) W[(size_t)r * nc + col[r]] = 1.0;
}

// pfwd(k): one workgroup per started panel (the grid).  acc = sum_j W_pj L_kj^T over the stored tiles (k, j), first[p] <= j < k, ascending; W_pk - acc, then
// sc_panel_kernel's substitution with L_kk.
__global__ __launch_bounds__(SC_THREADS) void sc_pfwd_kernel(const double* __restrict__ T, ScDev P, int k, int nc, double* __restrict__ W, const int32_t* __restrict__ first) {
    __shared__ double l[DC_NB * DC_LD];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lr = lane & 15, lk = lane >> 4;
    const int p = (int)blockIdx.x, fp = first[p];
    double* __restrict__ wrow = W + ((size_t)p * DC_NB + wave * DC_SUB + lr) * nc;
    const int diag = P.row_ptr[k + 1] - 1;
    sc_d4 acc[DC_NB / DC_SUB];
#pragma unroll
    for (int jb = 0; jb < DC_NB / DC_SUB; ++jb) acc[jb] = sc_d4{0.0, 0.0, 0.0, 0.0};
    for (int id = P.row_ptr[k]; id < diag; ++id) {
        const int j = P.row_col[id];
        if (j < fp) continue;                                              // (the same for every thread of the workgroup) W_pj is all zero
        __syncthreads();                                                   // the products of the tile before are done with l
        sc_load_tile(T + (size_t)id * SC_TILE, l);
        __syncthreads();
        const double* __restrict__ wj = wrow + (size_t)j * DC_NB;
#pragma unroll
        for (int kk = 0; kk < DC_NB / 4; ++kk) {
            const double b = wj[kk * 4 + lk];
#pragma unroll
            for (int jb = 0; jb < DC_NB / DC_SUB; ++jb) acc[jb] = __builtin_amdgcn_mfma_f64_16x16x4f64(l[(jb * DC_SUB + lr) * DC_LD + kk * 4 + lk], b, acc[jb], 0, 0, 0);
        }
    }
    __syncthreads();
    sc_load_tile(T + (size_t)diag * SC_TILE, l);
    __syncthreads();
    double* __restrict__ arow = wrow + (size_t)k * DC_NB;
    sc_d4 Y[DC_NB / DC_SUB];
#pragma unroll
    for (int j = 0; j < DC_NB / DC_SUB; ++j) {
        double r[4];
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) r[reg] = arow[j * DC_SUB + lk + 4 * reg] - acc[j][reg];
        sc_d4 sub = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int m = 0; m < j; ++m)
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
                sub = __builtin_amdgcn_mfma_f64_16x16x4f64(l[(j * DC_SUB + lr) * DC_LD + m * DC_SUB + 4 * kk + lk], Y[m][kk], sub, 0, 0, 0);
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) r[reg] = r[reg] - sub[reg];
#pragma unroll
        for (int q = 0; q < DC_SUB; ++q) {
            const double yq = __shfl(r[q >> 2], (q & 3) * 16 + lr) / l[(j * DC_SUB + q) * DC_LD + j * DC_SUB + q];
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int c = lk + 4 * reg;
                const double lcq = l[(j * DC_SUB + (c > q ? c : q)) * DC_LD + j * DC_SUB + q];      // (c <= q: the diagonal entry, unused)
                r[reg] = c == q ? yq : (c > q ? r[reg] - lcq * yq : r[reg]);
            }
        }
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            Y[j][reg] = r[reg];
            arow[j * DC_SUB + lk + 4 * reg] = r[reg];
        }
    }
}

// pbwd(k): one workgroup per panel (the grid).  acc = sum_{i in s_k} W_pi L_ik, i ascending; W_pk - acc, then sc_sel_ginv_kernel's substitution with L_kk.
__global__ __launch_bounds__(SC_THREADS) void sc_pbwd_kernel(const double* __restrict__ T, ScDev P, int k, int nc, double* __restrict__ W) {
    __shared__ double l[DC_NB * DC_LD];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lr = lane & 15, lk = lane >> 4;
    double* __restrict__ wrow = W + ((size_t)blockIdx.x * DC_NB + wave * DC_SUB + lr) * nc;
    sc_d4 acc[DC_NB / DC_SUB];
#pragma unroll
    for (int jb = 0; jb < DC_NB / DC_SUB; ++jb) acc[jb] = sc_d4{0.0, 0.0, 0.0, 0.0};
    for (int e = P.col_ptr[k]; e < P.col_ptr[k + 1]; ++e) {
        __syncthreads();                                                   // the products of the tile before are done with l
        sc_load_tile(T + (size_t)P.col_tile[e] * SC_TILE, l);
        __syncthreads();
        const double* __restrict__ wi = wrow + (size_t)P.col_row[e] * DC_NB;
#pragma unroll
        for (int kk = 0; kk < DC_NB / 4; ++kk) {
            const double b = wi[kk * 4 + lk];
#pragma unroll
            for (int jb = 0; jb < DC_NB / DC_SUB; ++jb) acc[jb] = __builtin_amdgcn_mfma_f64_16x16x4f64(l[(kk * 4 + lk) * DC_LD + jb * DC_SUB + lr], b, acc[jb], 0, 0, 0);
        }
    }
    __syncthreads();
    sc_load_tile(T + (size_t)(P.row_ptr[k + 1] - 1) * SC_TILE, l);
    __syncthreads();
    double* __restrict__ arow = wrow + (size_t)k * DC_NB;
    sc_d4 Y[DC_NB / DC_SUB];
#pragma unroll
    for (int j = DC_NB / DC_SUB - 1; j >= 0; --j) {
        double r[4];
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) r[reg] = arow[j * DC_SUB + lk + 4 * reg] - acc[j][reg];
        sc_d4 sub = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int m = DC_NB / DC_SUB - 1; m > j; --m)
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
                sub = __builtin_amdgcn_mfma_f64_16x16x4f64(l[(m * DC_SUB + 4 * kk + lk) * DC_LD + j * DC_SUB + lr], Y[m][kk], sub, 0, 0, 0);
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) r[reg] = r[reg] - sub[reg];
#pragma unroll
        for (int q = DC_SUB - 1; q >= 0; --q) {
            const double gq = __shfl(r[q >> 2], (q & 3) * 16 + lr) / l[(j * DC_SUB + q) * DC_LD + j * DC_SUB + q];
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int c = lk + 4 * reg;
                const double lqc = l[(j * DC_SUB + q) * DC_LD + j * DC_SUB + (c < q ? c : q)];      // (c >= q: the diagonal entry, unused)
                r[reg] = c == q ? gq : (c < q ? r[reg] - lqc * gq : r[reg]);
            }
        }
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            Y[j][reg] = r[reg];
            arow[j * DC_SUB + lk + 4 * reg] = r[reg];
        }
    }
}

// gather: one thread per entry of a requested block out of one chunk's W: entry (i, j) = row 6 pos[row keyframe] + i of the solution of right-hand side j of the column
// keyframe (sc_columns_gather_host).  row0[c] < 0: the column has no rows in this chunk — another chunk's, or a block with a keyframe outside the system, which stays
// as the zero it was set to.
__global__ __launch_bounds__(SC_THREADS) void sc_pgather_kernel(const double* __restrict__ W, int nc, int64_t n_blocks, const int32_t* __restrict__ row_node, const int32_t* __restrict__ col_index,
                                                                const int32_t* __restrict__ row0, const uint8_t* __restrict__ in_system, const int32_t* __restrict__ pos, double* __restrict__ out) {
    const int64_t gid = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x, blk = gid / 36;
    if (blk >= n_blocks) return;
    const int e = (int)(gid - blk * 36), i = e / 6, j = e - i * 6;
    const int32_t a = row_node[blk], r0 = row0[col_index[blk]];            // both in range: the host checked
    if (r0 < 0 || !in_system[a]) return;
    out[gid] = W[(size_t)(r0 + j) * nc + (size_t)pos[a] * 6 + i];
}

// ---- host side
thread_local std::string g_err;    // the last error of a call without an object

struct DevBuf {
    void* p = nullptr; size_t bytes = 0;
    hipError_t ensure(size_t b) {
        if (b <= bytes && p) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr; bytes = 0;
        const hipError_t e = hipMalloc(&p, b ? b : 8);
        if (e == hipSuccess) bytes = b ? b : 8; else p = nullptr;
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
    template <class V> V* as() const { return static_cast<V*>(p); }
};

#define SCHIP(err, call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) { (err) = std::string(#call) + ": " + hipGetErrorString(e_); return e_ == hipErrorOutOfMemory ? PGO_ERR_OUT_OF_MEMORY : PGO_ERR_HIP; } } while (0)

// the launches, walked by sc_factor_steps and sc_solve_steps.  first_forward: the forward steps before it are skipped (they would solve and subtract +0); with_backward
// = false: the forward sweep alone
struct ScLaunch {
    double* T; ScDev D; const ScPlan* P; double* LT; int32_t* fail; int nc; unsigned n_rhs; double* w; double* yv; double* x; int first_forward; bool with_backward; hipStream_t st;
    void factor_diag(int k, bool) { hipLaunchKernelGGL(sc_diag_kernel, dim3(1), dim3(SC_THREADS), 0, st, T, P->diag(k), fail); }
    void panel(int k) { hipLaunchKernelGGL(sc_panel_kernel, dim3((unsigned)P->s_size(k)), dim3(SC_THREADS), 0, st, T, D, k, P->ldu(), LT); }
    void update(int k) { const unsigned m = (unsigned)P->s_size(k); hipLaunchKernelGGL(sc_update_kernel, dim3(m * (m + 1) / 2), dim3(SC_THREADS), 0, st, T, D, k, P->ldu(), (const double*)LT, fail); }
    void forward(int k) { if (k >= first_forward) hipLaunchKernelGGL(sc_forward_kernel, dim3((unsigned)(1 + P->s_size(k)), n_rhs), dim3(SC_THREADS), 0, st, (const double*)T, D, k, nc, w, yv); }
    void backward(int k) {
        if (with_backward) hipLaunchKernelGGL(sc_backward_kernel, dim3((unsigned)(P->row_ptr[(size_t)k + 1] - P->row_ptr[(size_t)k]), n_rhs), dim3(SC_THREADS), 0, st, (const double*)T, D, k, nc, yv, x);
    }
};

// the launches of the selected inverse, walked by sc_selinv_steps.  G: the panel scratch (ScPlan::scratch_doubles() holds max |s_k| tiles)
struct ScSelLaunch {
    const double* T; double* Z; ScDev D; const ScPlan* P; double* G; hipStream_t st;
    void ginv(int k) { hipLaunchKernelGGL(sc_sel_ginv_kernel, dim3((unsigned)P->s_size(k)), dim3(SC_THREADS), 0, st, T, D, k, G); }
    void column(int k) { hipLaunchKernelGGL(sc_sel_column_kernel, dim3((unsigned)P->s_size(k)), dim3(SC_THREADS), 0, st, Z, D, k, (const double*)G); }
    void diag(int k) { hipLaunchKernelGGL(sc_sel_diag_kernel, dim3(1), dim3(SC_THREADS), 0, st, Z, D, k, (const double*)G); }
    void inverses() { hipLaunchKernelGGL(sc_sel_inverses_kernel, dim3((unsigned)P->nt), dim3(SC_THREADS), 0, st, T, Z, D); }
};

// the launches of the panel sweeps, walked by sc_panel_steps
struct ScPanelLaunch {
    const double* T; ScDev D; int nc; double* W; const int32_t* first; hipStream_t st;
    void pfwd(int k, int started) { hipLaunchKernelGGL(sc_pfwd_kernel, dim3((unsigned)started), dim3(SC_THREADS), 0, st, T, D, k, nc, W, first); }
    void pbwd(int k, int panels) { hipLaunchKernelGGL(sc_pbwd_kernel, dim3((unsigned)panels), dim3(SC_THREADS), 0, st, T, D, k, nc, W); }
};

// a device, a stream, a plan with its tables, tile storage and panel scratch
struct ScCore {
    int device = -1; hipStream_t st = nullptr; hipEvent_t e0 = nullptr, e1 = nullptr;
    ScPlan P; ScDev D{}; DevBuf tables, T, LT, vec, fail;
    std::string err;
    double last_ms = 0.0;
    int nc() const { return P.nt * DC_NB; }
    int open(int device_id) {
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess || count < 1) { err = "no HIP device"; return PGO_ERR_NO_DEVICE; }
        if (device_id == -1 && hipGetDevice(&device_id) != hipSuccess) { err = "no current HIP device"; return PGO_ERR_NO_DEVICE; }      // (pgo_options.device_id's convention)
        if (device_id < 0 || device_id >= count) { err = "no such HIP device"; return PGO_ERR_NO_DEVICE; }
        SCHIP(err, hipSetDevice(device_id));
        device = device_id;
        SCHIP(err, hipStreamCreate(&st));
        SCHIP(err, hipEventCreate(&e0)); SCHIP(err, hipEventCreate(&e1));
        return PGO_OK;
    }
    int use() { SCHIP(err, hipSetDevice(device)); return PGO_OK; }
    // the plan's six tables as int32, one upload; tile storage, scratch, failure flag
    int upload_plan() {
        std::vector<int32_t> h;
        size_t at[6];
        const std::vector<int32_t> ahead(P.ahead.begin(), P.ahead.end());
        const std::vector<int32_t>* parts[6] = {&P.row_ptr, &P.row_col, &P.col_ptr, &P.col_row, &P.col_tile, &ahead};
        for (int k = 0; k < 6; ++k) { at[k] = h.size(); h.insert(h.end(), parts[k]->begin(), parts[k]->end()); }
        SCHIP(err, tables.ensure(h.size() * sizeof(int32_t)));
        SCHIP(err, hipMemcpy(tables.p, h.data(), h.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        const int32_t* d = tables.as<int32_t>();
        D = ScDev{d + at[0], d + at[1], d + at[2], d + at[3], d + at[4], d + at[5]};
        SCHIP(err, T.ensure((size_t)P.tiles() * SC_TILE * sizeof(double)));
        SCHIP(err, LT.ensure(P.scratch_doubles() * sizeof(double)));
        SCHIP(err, fail.ensure(sizeof(int32_t)));
        return PGO_OK;
    }
    ScLaunch launcher(unsigned n_rhs, double* w, double* yv, double* x, int first_forward, bool with_backward) {
        return ScLaunch{T.as<double>(), D, &P, LT.as<double>(), fail.as<int32_t>(), nc(), n_rhs, w, yv, x, first_forward, with_backward, st};
    }
    // after a run of launches between e0 and e1: the stream's end, the launches' errors, the events' time
    int finish() {
        SCHIP(err, hipStreamSynchronize(st));
        SCHIP(err, hipGetLastError());
        float ms = 0;
        SCHIP(err, hipEventElapsedTime(&ms, e0, e1));
        last_ms = ms;
        return PGO_OK;
    }
    void close() {
        if (device < 0) return;
        (void)hipSetDevice(device);
        if (st) (void)hipStreamSynchronize(st);
        for (DevBuf* b : {&tables, &T, &LT, &vec, &fail}) b->release();
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        if (st) (void)hipStreamDestroy(st);
        st = nullptr; e0 = e1 = nullptr; device = -1;
    }
};

void plan_info(const ScPlan& P, int used, int64_t* info8) {
    const int64_t v[8] = {P.nt, P.a_tiles, P.tiles(), used, (int64_t)(P.tiles() * (int64_t)SC_TILE * 8), P.factor_launches(), P.solve_launches(), P.tile_updates()};
    std::copy(v, v + 8, info8);
}

}  // namespace

}  // namespace pgo

using namespace pgo;

struct pgo_sparse_chol {
    ScCore c;
    int64_t N = 0, n_pairs = 0;
    int used = 0;
    bool factored = false;
    bool selected = false;      // Z holds the selected inverse of the present factor
    std::vector<uint8_t> in_system;
    std::vector<int32_t> order, pos;
    std::vector<int32_t> h_hi, h_lo;                       // the pair list as pgo_sparse_chol_create took it (pgo_sparse_lm_create reads it)
    DevBuf d_in, d_pos, d_hi, d_lo, d_diag, d_blocks, d_at, d_val, d_pr, d_out, Z, d_na, d_nb, d_flag;
    DevBuf ws, d_req;                                      // pgo_sparse_chol_inverse_columns: W of one chunk, the chunk's tables
    int64_t ws_limit = PGO_SPARSE_WORKSPACE_BYTES;
    int64_t cols_info[4] = {0, 0, 0, 0};                   // of the last pgo_sparse_chol_inverse_columns
    void release() {
        if (c.device >= 0) (void)hipSetDevice(c.device);
        if (c.st) (void)hipStreamSynchronize(c.st);
        for (DevBuf* b : {&d_in, &d_pos, &d_hi, &d_lo, &d_diag, &d_blocks, &d_at, &d_val, &d_pr, &d_out, &Z, &d_na, &d_nb, &d_flag, &ws, &d_req}) b->release();
        c.close();
    }
};

extern "C" {

const char* pgo_sparse_strerror(int code) {
    switch (code) {
        case PGO_OK: return "ok";
        case PGO_ERR_INVALID_ARG: return "invalid argument";
        case PGO_ERR_NO_DEVICE: return "no HIP device";
        case PGO_ERR_HIP: return "a HIP call failed";
        case PGO_ERR_OUT_OF_MEMORY: return "out of device memory";
        case PGO_ERR_STATE: return "call order violated";
        case PGO_ERR_NUMERIC: return "the matrix is not numerically positive definite";
        default: return "unknown error";
    }
}
const char* pgo_sparse_last_error(const pgo_sparse_chol* h) { return h ? h->c.err.c_str() : g_err.c_str(); }

int pgo_sparse_spd_solve(int32_t device_id, int32_t n, const double* a, const double* b, const int32_t* pos, double* x, int64_t* info8, int32_t launches, double* avg_ms) {
    g_err.clear();
    if (n <= 0 || n > (1 << 30) || !a || !b || !x || launches < 1) { g_err = "pgo_sparse_spd_solve: null pointer, n <= 0 or launches < 1"; return PGO_ERR_INVALID_ARG; }
    if (pos) {
        std::vector<uint8_t> seen((size_t)n, 0);
        for (int i = 0; i < n; ++i) { if (pos[i] < 0 || pos[i] >= n || seen[(size_t)pos[i]]) { g_err = "pgo_sparse_spd_solve: pos is not a permutation of 0 .. n - 1"; return PGO_ERR_INVALID_ARG; } seen[(size_t)pos[i]] = 1; }
    }
    ScCore c;
    struct Closer { ScCore& c; ~Closer() { g_err = c.err; c.close(); } } closer{c};
    int rc;
    if ((rc = c.open(device_id)) != PGO_OK) return rc;
    c.P = sc_plan_matrix(n, a, pos);
    if (info8) plan_info(c.P, 0, info8);
    if ((rc = c.upload_plan()) != PGO_OK) return rc;
    const int nc = c.nc();
    std::vector<double> hT((size_t)c.P.tiles() * SC_TILE, 0.0), hw((size_t)nc, 0.0);
    sc_fill_tiles(c.P, n, a, pos, hT.data());
    for (int i = 0; i < n; ++i) hw[(size_t)(pos ? pos[i] : i)] = b[i];
    SCHIP(c.err, c.vec.ensure((size_t)3 * nc * sizeof(double)));
    double* w = c.vec.as<double>();
    ScLaunch L = c.launcher(1, w, w + nc, w + 2 * (size_t)nc, 0, true);
    double total = 0.0;
    int32_t fail = 0;
    for (int l = 0; l < launches && !fail; ++l) {
        SCHIP(c.err, hipMemcpyAsync(c.T.p, hT.data(), hT.size() * sizeof(double), hipMemcpyHostToDevice, c.st));
        SCHIP(c.err, hipMemcpyAsync(w, hw.data(), hw.size() * sizeof(double), hipMemcpyHostToDevice, c.st));
        SCHIP(c.err, hipMemsetAsync(c.fail.p, 0, sizeof(int32_t), c.st));
        SCHIP(c.err, hipEventRecord(c.e0, c.st));
        sc_factor_steps(c.P, L);
        sc_solve_steps(c.P, L);      // (a failed factor: the sweeps run on numbers nobody reads — every address comes from the plan, none from the numbers)
        SCHIP(c.err, hipEventRecord(c.e1, c.st));
        SCHIP(c.err, hipMemcpyAsync(&fail, c.fail.p, sizeof(fail), hipMemcpyDeviceToHost, c.st));
        if ((rc = c.finish()) != PGO_OK) return rc;
        total += c.last_ms;
    }
    if (avg_ms) *avg_ms = total / launches;
    if (fail) { c.err = "pgo_sparse_spd_solve: the matrix is not numerically positive definite"; return PGO_ERR_NUMERIC; }
    SCHIP(c.err, hipMemcpy(hw.data(), w + 2 * (size_t)nc, hw.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) x[i] = hw[(size_t)(pos ? pos[i] : i)];
    return PGO_OK;
}

int pgo_sparse_chol_create(int32_t device_id, int64_t n_nodes, const uint8_t* in_system, int64_t n_pairs, const int32_t* pair_hi, const int32_t* pair_lo, int32_t ordering, pgo_sparse_chol** out) {
    g_err.clear();
    if (!out) { g_err = "pgo_sparse_chol_create: null pointer"; return PGO_ERR_INVALID_ARG; }
    *out = nullptr;
    if (n_nodes < 1 || n_nodes > (int64_t)300000000 || !in_system || n_pairs < 0 || (n_pairs > 0 && (!pair_hi || !pair_lo)) || ordering < -1 || ordering > 1) {
        g_err = "pgo_sparse_chol_create: null pointer, count out of range or unknown ordering"; return PGO_ERR_INVALID_ARG;
    }
    if (const char* what = sc_check_pairs(n_nodes, in_system, n_pairs, pair_hi, pair_lo)) { g_err = std::string("pgo_sparse_chol_create: ") + what; return PGO_ERR_INVALID_ARG; }
    pgo_sparse_chol* h = new pgo_sparse_chol;
    struct Guard { pgo_sparse_chol* h; ~Guard() { if (h) { g_err = h->c.err; h->release(); delete h; } } } guard{h};
    int rc;
    if ((rc = h->c.open(device_id)) != PGO_OK) return rc;
    h->N = n_nodes; h->n_pairs = n_pairs;
    h->in_system.assign(in_system, in_system + n_nodes);
    if (n_pairs) { h->h_hi.assign(pair_hi, pair_hi + n_pairs); h->h_lo.assign(pair_lo, pair_lo + n_pairs); }
    std::vector<int64_t> adj_ptr; std::vector<int32_t> adj;
    sc_pair_adjacency(n_nodes, n_pairs, pair_hi, pair_lo, adj_ptr, adj);
    h->c.P = sc_plan_graph(n_nodes, adj_ptr.data(), adj.data(), in_system, ordering, h->order, &h->used);
    h->pos.assign((size_t)n_nodes, 0);
    for (int64_t q = 0; q < n_nodes; ++q) h->pos[(size_t)h->order[(size_t)q]] = (int32_t)q;
    if ((rc = h->c.upload_plan()) != PGO_OK) return rc;
    ScCore& c = h->c;
    SCHIP(c.err, h->d_in.ensure((size_t)n_nodes)); SCHIP(c.err, h->d_pos.ensure((size_t)n_nodes * sizeof(int32_t)));
    SCHIP(c.err, h->d_hi.ensure((size_t)n_pairs * sizeof(int32_t))); SCHIP(c.err, h->d_lo.ensure((size_t)n_pairs * sizeof(int32_t)));
    SCHIP(c.err, h->d_diag.ensure((size_t)n_nodes * 36 * sizeof(double))); SCHIP(c.err, h->d_blocks.ensure((size_t)n_pairs * 36 * sizeof(double)));
    SCHIP(c.err, hipMemcpy(h->d_in.p, in_system, (size_t)n_nodes, hipMemcpyHostToDevice));
    SCHIP(c.err, hipMemcpy(h->d_pos.p, h->pos.data(), (size_t)n_nodes * sizeof(int32_t), hipMemcpyHostToDevice));
    if (n_pairs) {
        SCHIP(c.err, hipMemcpy(h->d_hi.p, pair_hi, (size_t)n_pairs * sizeof(int32_t), hipMemcpyHostToDevice));
        SCHIP(c.err, hipMemcpy(h->d_lo.p, pair_lo, (size_t)n_pairs * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    guard.h = nullptr;
    *out = h;
    return PGO_OK;
}

void pgo_sparse_chol_destroy(pgo_sparse_chol* h) {
    if (!h) return;
    h->release();
    delete h;
}

int pgo_sparse_chol_info(const pgo_sparse_chol* h, int64_t* info8, int32_t* order) {
    if (!h) return PGO_ERR_INVALID_ARG;
    if (info8) plan_info(h->c.P, h->used, info8);
    if (order) std::copy(h->order.begin(), h->order.end(), order);
    return PGO_OK;
}

double pgo_sparse_chol_last_ms(const pgo_sparse_chol* h) { return h ? h->c.last_ms : 0.0; }

int pgo_sparse_chol_factor(pgo_sparse_chol* h, const double* diag, const double* pair_blocks) {
    if (!h) return PGO_ERR_INVALID_ARG;
    ScCore& c = h->c;
    c.err.clear();
    if (!diag || (h->n_pairs > 0 && !pair_blocks)) { c.err = "pgo_sparse_chol_factor: null pointer"; return PGO_ERR_INVALID_ARG; }
    int rc;
    if ((rc = c.use()) != PGO_OK) return rc;
    h->factored = false;
    h->selected = false;      // (Z, if there is one, belongs to the factor before)
    const int nc = c.nc();
    SCHIP(c.err, hipMemcpyAsync(h->d_diag.p, diag, (size_t)h->N * 36 * sizeof(double), hipMemcpyHostToDevice, c.st));
    if (h->n_pairs) SCHIP(c.err, hipMemcpyAsync(h->d_blocks.p, pair_blocks, (size_t)h->n_pairs * 36 * sizeof(double), hipMemcpyHostToDevice, c.st));
    SCHIP(c.err, hipMemsetAsync(c.fail.p, 0, sizeof(int32_t), c.st));
    SCHIP(c.err, hipEventRecord(c.e0, c.st));
    SCHIP(c.err, hipMemsetAsync(c.T.p, 0, (size_t)c.P.tiles() * SC_TILE * sizeof(double), c.st));
    const int64_t threads = h->N * 36 + ((int64_t)nc - h->N * 6) + h->n_pairs * 36;
    hipLaunchKernelGGL(sc_fill_kernel, dim3((unsigned)((threads + SC_THREADS - 1) / SC_THREADS)), dim3(SC_THREADS), 0, c.st, c.T.as<double>(), c.D, h->N, nc, h->d_in.as<const uint8_t>(),
                       h->d_pos.as<const int32_t>(), h->d_diag.as<const double>(), h->n_pairs, h->d_hi.as<const int32_t>(), h->d_lo.as<const int32_t>(), h->d_blocks.as<const double>());
    ScLaunch L = c.launcher(1, nullptr, nullptr, nullptr, 0, false);
    sc_factor_steps(c.P, L);
    SCHIP(c.err, hipEventRecord(c.e1, c.st));
    int32_t fail = 1;
    SCHIP(c.err, hipMemcpyAsync(&fail, c.fail.p, sizeof(fail), hipMemcpyDeviceToHost, c.st));
    if ((rc = c.finish()) != PGO_OK) return rc;
    if (fail) { c.err = "pgo_sparse_chol_factor: the matrix is not numerically positive definite"; return PGO_ERR_NUMERIC; }
    h->factored = true;
    return PGO_OK;
}

int pgo_sparse_chol_solve(pgo_sparse_chol* h, int64_t n_rhs, const double* B, double* X) {
    if (!h) return PGO_ERR_INVALID_ARG;
    ScCore& c = h->c;
    c.err.clear();
    if (n_rhs < 1 || n_rhs > PGO_SPARSE_MAX_RHS || !B || !X) { c.err = "pgo_sparse_chol_solve: null pointer, or n_rhs outside 1 .. PGO_SPARSE_MAX_RHS"; return PGO_ERR_INVALID_ARG; }
    if (!h->factored) { c.err = "pgo_sparse_chol_solve: no factor (pgo_sparse_chol_factor has not succeeded)"; return PGO_ERR_STATE; }
    int rc;
    if ((rc = c.use()) != PGO_OK) return rc;
    const size_t nc = (size_t)c.nc(), n6 = (size_t)h->N * 6, total = (size_t)n_rhs * nc;
    std::vector<double> hw(total, 0.0);
    for (int64_t r = 0; r < n_rhs; ++r)
        for (int64_t i = 0; i < h->N; ++i)
            if (h->in_system[(size_t)i]) std::memcpy(&hw[(size_t)r * nc + (size_t)h->pos[(size_t)i] * 6], B + (size_t)r * n6 + (size_t)i * 6, 6 * sizeof(double));
    SCHIP(c.err, c.vec.ensure(3 * total * sizeof(double)));
    double* w = c.vec.as<double>();
    SCHIP(c.err, hipMemcpyAsync(w, hw.data(), total * sizeof(double), hipMemcpyHostToDevice, c.st));
    ScLaunch L = c.launcher((unsigned)n_rhs, w, w + total, w + 2 * total, 0, true);
    SCHIP(c.err, hipEventRecord(c.e0, c.st));
    sc_solve_steps(c.P, L);
    SCHIP(c.err, hipEventRecord(c.e1, c.st));
    SCHIP(c.err, hipMemcpyAsync(hw.data(), w + 2 * total, total * sizeof(double), hipMemcpyDeviceToHost, c.st));
    if ((rc = c.finish()) != PGO_OK) return rc;
    for (int64_t r = 0; r < n_rhs; ++r)
        for (int64_t i = 0; i < h->N; ++i) {
            double* xo = X + (size_t)r * n6 + (size_t)i * 6;
            if (h->in_system[(size_t)i]) std::memcpy(xo, &hw[(size_t)r * nc + (size_t)h->pos[(size_t)i] * 6], 6 * sizeof(double));
            else std::fill(xo, xo + 6, 0.0);
        }
    return PGO_OK;
}

int pgo_sparse_chol_inverse_blocks(pgo_sparse_chol* h, int64_t n_groups, const int64_t* group_ptr, const int64_t* row_ptr, const int32_t* col, const double* val,
                                   int64_t n_pairs, const int32_t* ga, const int32_t* gb, double* out) {
    if (!h) return PGO_ERR_INVALID_ARG;
    ScCore& c = h->c;
    c.err.clear();
    if (n_groups < 1 || n_groups > PGO_SPARSE_MAX_GROUPS) { c.err = "pgo_sparse_chol_inverse_blocks: the number of groups is outside 1 .. PGO_SPARSE_MAX_GROUPS"; return PGO_ERR_INVALID_ARG; }
    if (!group_ptr || !row_ptr || n_pairs < 0 || (n_pairs > 0 && (!ga || !gb || !out))) { c.err = "pgo_sparse_chol_inverse_blocks: null pointer or negative count"; return PGO_ERR_INVALID_ARG; }
    for (int64_t k = 0; k < n_pairs; ++k) if (ga[k] < 0 || ga[k] >= n_groups || gb[k] < 0 || gb[k] >= n_groups) { c.err = "pgo_sparse_chol_inverse_blocks: a pair names a group out of range"; return PGO_ERR_INVALID_ARG; }
    if (!h->factored) { c.err = "pgo_sparse_chol_inverse_blocks: no factor (pgo_sparse_chol_factor has not succeeded)"; return PGO_ERR_STATE; }
    const int nc = c.nc();
    const ScRows R(h->N, h->in_system.data(), h->pos.data(), nc, n_groups, group_ptr, row_ptr, col, val);
    if (R.error) { c.err = std::string("pgo_sparse_chol_inverse_blocks: ") + R.error; return PGO_ERR_INVALID_ARG; }
    if (n_pairs == 0) return PGO_OK;
    int rc;
    if ((rc = c.use()) != PGO_OK) return rc;
    const size_t total = (size_t)R.rows * nc, nnz = R.at.size();
    std::vector<int32_t> pr;
    for (int64_t k = 0; k < n_pairs; ++k) for (int32_t v : {R.first_row[(size_t)ga[k]], R.first_row[(size_t)gb[k]], R.dim[(size_t)ga[k]] | (R.dim[(size_t)gb[k]] << 8)}) pr.push_back(v);
    SCHIP(c.err, c.vec.ensure(2 * total * sizeof(double)));
    SCHIP(c.err, h->d_at.ensure(nnz * sizeof(int64_t))); SCHIP(c.err, h->d_val.ensure(nnz * sizeof(double)));
    SCHIP(c.err, h->d_pr.ensure(pr.size() * sizeof(int32_t))); SCHIP(c.err, h->d_out.ensure((size_t)n_pairs * 36 * sizeof(double)));
    double* w = c.vec.as<double>();
    double* yv = w + total;
    if (nnz) {
        SCHIP(c.err, hipMemcpyAsync(h->d_at.p, R.at.data(), nnz * sizeof(int64_t), hipMemcpyHostToDevice, c.st));
        SCHIP(c.err, hipMemcpyAsync(h->d_val.p, R.val.data(), nnz * sizeof(double), hipMemcpyHostToDevice, c.st));
    }
    SCHIP(c.err, hipMemcpyAsync(h->d_pr.p, pr.data(), pr.size() * sizeof(int32_t), hipMemcpyHostToDevice, c.st));
    SCHIP(c.err, hipEventRecord(c.e0, c.st));
    SCHIP(c.err, hipMemsetAsync(w, 0, 2 * total * sizeof(double), c.st));      // (y of the skipped steps: the zeros the Gram products read as such)
    if (nnz) hipLaunchKernelGGL(sc_rhs_kernel, dim3((unsigned)((nnz + SC_THREADS - 1) / SC_THREADS)), dim3(SC_THREADS), 0, c.st, w, (int64_t)nnz, h->d_at.as<const int64_t>(), h->d_val.as<const double>());
    ScLaunch L = c.launcher((unsigned)R.rows, w, yv, nullptr, R.first_tile, false);
    sc_solve_steps(c.P, L);
    const int c0 = std::min(R.first_tile * DC_NB, nc) / DC_GRAM * DC_GRAM;      // every column before it holds zeros in every row
    hipLaunchKernelGGL(sc_gram_kernel, dim3((unsigned)n_pairs), dim3(SC_THREADS), 0, c.st, (const double*)yv, nc, c0, h->d_pr.as<const int32_t>(), h->d_out.as<double>());
    SCHIP(c.err, hipEventRecord(c.e1, c.st));
    std::vector<double> blocks((size_t)n_pairs * 36);
    SCHIP(c.err, hipMemcpyAsync(blocks.data(), h->d_out.p, blocks.size() * sizeof(double), hipMemcpyDeviceToHost, c.st));
    if ((rc = c.finish()) != PGO_OK) return rc;
    std::copy(blocks.begin(), blocks.end(), out);
    return PGO_OK;
}

int pgo_sparse_chol_selected_inverse(pgo_sparse_chol* h) {
    if (!h) return PGO_ERR_INVALID_ARG;
    ScCore& c = h->c;
    c.err.clear();
    if (!h->factored) { c.err = "pgo_sparse_chol_selected_inverse: no factor (pgo_sparse_chol_factor has not succeeded)"; return PGO_ERR_STATE; }
    int rc;
    if ((rc = c.use()) != PGO_OK) return rc;
    h->selected = false;
    SCHIP(c.err, h->Z.ensure((size_t)c.P.tiles() * SC_TILE * sizeof(double)));      // (every tile is written by the step of its column: no memset)
    ScSelLaunch L{c.T.as<const double>(), h->Z.as<double>(), c.D, &c.P, c.LT.as<double>(), c.st};
    SCHIP(c.err, hipEventRecord(c.e0, c.st));
    sc_selinv_steps(c.P, L);
    SCHIP(c.err, hipEventRecord(c.e1, c.st));
    if ((rc = c.finish()) != PGO_OK) return rc;
    h->selected = true;
    return PGO_OK;
}

int pgo_sparse_chol_selected_info(const pgo_sparse_chol* h, int64_t* info4) {
    if (!h || !info4) return PGO_ERR_INVALID_ARG;
    const ScPlan& P = h->c.P;
    const int64_t v[4] = {P.selinv_launches(), P.selinv_products(), (int64_t)(P.tiles() * (int64_t)SC_TILE * 8), h->selected ? 1 : 0};
    std::copy(v, v + 4, info4);
    return PGO_OK;
}

int pgo_sparse_chol_selected_blocks(pgo_sparse_chol* h, int64_t n_blocks, const int32_t* node_a, const int32_t* node_b, double* out, uint8_t* in_pattern) {
    if (!h) return PGO_ERR_INVALID_ARG;
    ScCore& c = h->c;
    c.err.clear();
    if (n_blocks < 0 || n_blocks > (int64_t)50000000 || (n_blocks > 0 && (!node_a || !node_b || !out))) { c.err = "pgo_sparse_chol_selected_blocks: null pointer or count out of range"; return PGO_ERR_INVALID_ARG; }
    for (int64_t k = 0; k < n_blocks; ++k)
        if (node_a[k] < 0 || node_a[k] >= h->N || node_b[k] < 0 || node_b[k] >= h->N) { c.err = "pgo_sparse_chol_selected_blocks: block " + std::to_string(k) + " names a keyframe out of range"; return PGO_ERR_INVALID_ARG; }
    if (!h->selected) { c.err = "pgo_sparse_chol_selected_blocks: no selected inverse of the present factor (pgo_sparse_chol_selected_inverse has not succeeded since the last pgo_sparse_chol_factor)"; return PGO_ERR_STATE; }
    if (n_blocks == 0) return PGO_OK;
    int rc;
    if ((rc = c.use()) != PGO_OK) return rc;
    const size_t nb = (size_t)n_blocks;
    SCHIP(c.err, h->d_na.ensure(nb * sizeof(int32_t))); SCHIP(c.err, h->d_nb.ensure(nb * sizeof(int32_t)));
    SCHIP(c.err, h->d_out.ensure(nb * 36 * sizeof(double))); SCHIP(c.err, h->d_flag.ensure(nb));
    SCHIP(c.err, hipMemcpyAsync(h->d_na.p, node_a, nb * sizeof(int32_t), hipMemcpyHostToDevice, c.st));
    SCHIP(c.err, hipMemcpyAsync(h->d_nb.p, node_b, nb * sizeof(int32_t), hipMemcpyHostToDevice, c.st));
    SCHIP(c.err, hipEventRecord(c.e0, c.st));
    hipLaunchKernelGGL(sc_sel_gather_kernel, dim3((unsigned)((nb * 36 + SC_THREADS - 1) / SC_THREADS)), dim3(SC_THREADS), 0, c.st, h->Z.as<const double>(), c.D, n_blocks, h->d_na.as<const int32_t>(),
                       h->d_nb.as<const int32_t>(), h->d_in.as<const uint8_t>(), h->d_pos.as<const int32_t>(), h->d_out.as<double>(), h->d_flag.as<uint8_t>());
    SCHIP(c.err, hipEventRecord(c.e1, c.st));
    std::vector<double> blocks(nb * 36);
    std::vector<uint8_t> flag(nb);
    SCHIP(c.err, hipMemcpyAsync(blocks.data(), h->d_out.p, blocks.size() * sizeof(double), hipMemcpyDeviceToHost, c.st));
    SCHIP(c.err, hipMemcpyAsync(flag.data(), h->d_flag.p, nb, hipMemcpyDeviceToHost, c.st));
    if ((rc = c.finish()) != PGO_OK) return rc;
    if (!in_pattern)
        for (size_t k = 0; k < nb; ++k)
            if (!flag[k]) {
                c.err = "pgo_sparse_chol_selected_blocks: block " + std::to_string(k) + " (keyframes " + std::to_string(node_a[k]) + ", " + std::to_string(node_b[k]) + ") is not wholly in the pattern of the factor";
                return PGO_ERR_INVALID_ARG;
            }
    std::copy(blocks.begin(), blocks.end(), out);
    if (in_pattern) std::copy(flag.begin(), flag.end(), in_pattern);
    return PGO_OK;
}

int pgo_sparse_chol_inverse_columns(pgo_sparse_chol* h, int64_t n_cols, const int32_t* col_node, int64_t n_blocks, const int32_t* row_node, const int32_t* col_index, double* out) {
    if (!h) return PGO_ERR_INVALID_ARG;
    ScCore& c = h->c;
    c.err.clear();
    if (n_cols < 0 || n_cols > h->N || n_blocks < 0 || n_blocks > (int64_t)50000000 || (n_cols > 0 && !col_node) || (n_blocks > 0 && (!row_node || !col_index || !out))) {
        c.err = "pgo_sparse_chol_inverse_columns: null pointer or count out of range"; return PGO_ERR_INVALID_ARG;
    }
    if (!h->factored) { c.err = "pgo_sparse_chol_inverse_columns: no factor (pgo_sparse_chol_factor has not succeeded)"; return PGO_ERR_STATE; }
    const int nc = c.nc();
    const ScColumns Q(c.P, h->N, h->in_system.data(), h->pos.data(), n_cols, col_node, n_blocks, row_node, col_index, h->ws_limit);
    if (Q.error) { c.err = std::string("pgo_sparse_chol_inverse_columns: ") + Q.error; return PGO_ERR_INVALID_ARG; }
    const int64_t info[4] = {Q.launches, Q.products, Q.workspace, (int64_t)Q.chunks.size()};
    std::copy(info, info + 4, h->cols_info);
    if (n_blocks == 0) return PGO_OK;
    int rc;
    if ((rc = c.use()) != PGO_OK) return rc;
    const size_t nb = (size_t)n_blocks;
    std::vector<int32_t> tab;                              // every chunk's tables, one upload: rhs_col | first | row0
    std::vector<size_t> at;
    for (const ScColumnChunk& C : Q.chunks) {
        at.push_back(tab.size());
        tab.insert(tab.end(), C.rhs_col.begin(), C.rhs_col.end());
        tab.insert(tab.end(), C.first.begin(), C.first.end());
        tab.insert(tab.end(), C.row0.begin(), C.row0.end());
    }
    SCHIP(c.err, h->ws.ensure((size_t)Q.workspace));
    SCHIP(c.err, h->d_req.ensure(tab.size() * sizeof(int32_t)));
    SCHIP(c.err, h->d_na.ensure(nb * sizeof(int32_t))); SCHIP(c.err, h->d_nb.ensure(nb * sizeof(int32_t)));
    SCHIP(c.err, h->d_out.ensure(nb * 36 * sizeof(double)));
    SCHIP(c.err, hipMemcpyAsync(h->d_na.p, row_node, nb * sizeof(int32_t), hipMemcpyHostToDevice, c.st));
    SCHIP(c.err, hipMemcpyAsync(h->d_nb.p, col_index, nb * sizeof(int32_t), hipMemcpyHostToDevice, c.st));
    if (!tab.empty()) SCHIP(c.err, hipMemcpyAsync(h->d_req.p, tab.data(), tab.size() * sizeof(int32_t), hipMemcpyHostToDevice, c.st));
    SCHIP(c.err, hipEventRecord(c.e0, c.st));
    SCHIP(c.err, hipMemsetAsync(h->d_out.p, 0, nb * 36 * sizeof(double), c.st));
    double* W = h->ws.as<double>();
    for (size_t q = 0; q < Q.chunks.size(); ++q) {
        const ScColumnChunk& C = Q.chunks[q];
        const int32_t* d_col = h->d_req.as<const int32_t>() + at[q];
        const int32_t* d_first = d_col + C.rhs_col.size();
        const int32_t* d_row0 = d_first + C.first.size();
        SCHIP(c.err, hipMemsetAsync(W, 0, (size_t)C.m_pad * nc * sizeof(double), c.st));
        hipLaunchKernelGGL(sc_pcol_rhs_kernel, dim3((unsigned)((C.m_pad + SC_THREADS - 1) / SC_THREADS)), dim3(SC_THREADS), 0, c.st, W, nc, C.m_pad, d_col);
        ScPanelLaunch L{c.T.as<const double>(), c.D, nc, W, d_first, c.st};
        sc_panel_steps(c.P, C.first, Q.k_stop, L);
        hipLaunchKernelGGL(sc_pgather_kernel, dim3((unsigned)((nb * 36 + SC_THREADS - 1) / SC_THREADS)), dim3(SC_THREADS), 0, c.st, (const double*)W, nc, n_blocks, h->d_na.as<const int32_t>(),
                           h->d_nb.as<const int32_t>(), d_row0, h->d_in.as<const uint8_t>(), h->d_pos.as<const int32_t>(), h->d_out.as<double>());
    }
    SCHIP(c.err, hipEventRecord(c.e1, c.st));
    std::vector<double> blocks(nb * 36);
    SCHIP(c.err, hipMemcpyAsync(blocks.data(), h->d_out.p, blocks.size() * sizeof(double), hipMemcpyDeviceToHost, c.st));
    if ((rc = c.finish()) != PGO_OK) return rc;
    std::copy(blocks.begin(), blocks.end(), out);
    return PGO_OK;
}

int pgo_sparse_chol_columns_info(const pgo_sparse_chol* h, int64_t* info4) {
    if (!h || !info4) return PGO_ERR_INVALID_ARG;
    std::copy(h->cols_info, h->cols_info + 4, info4);
    return PGO_OK;
}

int pgo_sparse_chol_set_workspace_limit(pgo_sparse_chol* h, int64_t bytes) {
    if (!h) return PGO_ERR_INVALID_ARG;
    h->c.err.clear();
    if (bytes < sc_panel_bytes(h->c.nc())) { h->c.err = "pgo_sparse_chol_set_workspace_limit: below one panel of right-hand sides, 64 rows of " + std::to_string(h->c.nc()) + " doubles"; return PGO_ERR_INVALID_ARG; }
    h->ws_limit = bytes;
    return PGO_OK;
}

int pgo_sparse_reduce_normal_blocks(int64_t n_nodes, const uint8_t* node_free, const double* diag, const double* offdiag, const double* sw_c, const double* sw_hss,
                                    int64_t n_rel, const int32_t* rel_c1, const int32_t* rel_c2, int64_t n_sw, const int32_t* swe_c1, const int32_t* swe_c2,
                                    int64_t* n_pairs, int32_t* pair_hi, int32_t* pair_lo, double* s_diag, double* s_blocks) {
    g_err.clear();
    const int64_t E = n_rel + n_sw;
    if (n_nodes < 1 || n_rel < 0 || n_sw < 0 || !node_free || !diag || !n_pairs || !s_diag || (E > 0 && (!offdiag || !pair_hi || !pair_lo || !s_blocks)) ||
        (n_rel > 0 && (!rel_c1 || !rel_c2)) || (n_sw > 0 && (!swe_c1 || !swe_c2 || !sw_c || !sw_hss))) {
        g_err = "pgo_sparse_reduce_normal_blocks: null pointer or negative count"; return PGO_ERR_INVALID_ARG;
    }
    const ScReduced R = sc_reduce_normal_blocks(n_nodes, node_free, diag, offdiag, sw_c, sw_hss, n_rel, rel_c1, rel_c2, n_sw, swe_c1, swe_c2);
    *n_pairs = (int64_t)R.pair_hi.size();
    std::copy(R.pair_hi.begin(), R.pair_hi.end(), pair_hi);
    std::copy(R.pair_lo.begin(), R.pair_lo.end(), pair_lo);
    std::copy(R.diag.begin(), R.diag.end(), s_diag);
    std::copy(R.blocks.begin(), R.blocks.end(), s_blocks);
    return PGO_OK;
}

}  // extern "C"

// the exact Levenberg-Marquardt step and solve on this factor (pgo_sparse_lm_*): kernels, object and entry points
#include "pgo_sparse_lm.hpp"
