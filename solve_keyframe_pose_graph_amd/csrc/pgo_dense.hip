// pgo_dense.hip — the exact dense linear solver (PGO_LINEAR_DENSE_CHOLESKY): the block-CSR system of an LM step scattered into a dense row-major matrix, a blocked
// right-looking Cholesky factorisation in place on its lower triangle, and the two triangular sweeps.  The algorithm, the block routines and the order of the block steps
// are pgo_dense_math.hpp's (which also runs them serially on the host); this file holds the kernels, their launchers and the handle's side of a dense step (dense_step).
//
// Launches of one system of order n = 64 nt:  1 (first diagonal block) + 2 (nt - 1) (panel, update) for the factor, 2 nt for the sweeps.  Nothing waits on another workgroup
// inside a launch, there are no atomics, and every sum has a fixed order.  All fp64; the panel's and the update's products run on v_mfma_f64_16x16x4_f64 (operand maps: the
// comment above gj_block_inverse in pgo_kernels.hip).
//
// Covariance blocks (pgo_pose_covariance and pgo_covariance, one path): 1 (the right-hand sides: a keyframe's six unit rows, a switch's row -c_e / h_e; dcp_rhs_kernel,
// ahead of the factor) + 2 (nt - k0) - 1 (solve, update from the first requested block column k0 on) + 1 (Gram products of 6- and 1-row blocks, dcp_gram_kernel)
// launches, under the same rules.  On a matrix-free graph the matrix comes from the normal blocks in one scatter launch (dcm_scatter_kernel) instead of build_rows +
// dc_scatter_kernel.
#include <algorithm>
#include <cstdlib>
#include <limits>

#include "pgo_handle.hpp"
#include "pgo_dense_math.hpp"
#include "pgo_tile_ops.hpp"

namespace pgo {

namespace {

constexpr int DC_THREADS = 256;

struct DcTeam {
    __device__ __forceinline__ int rank() const { return (int)threadIdx.x; }
    __device__ __forceinline__ int size() const { return DC_THREADS; }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
};

// the 64 x 64 block at (k0, k0) -> LDS, all of it (the part above the diagonal is never read)
__device__ __forceinline__ void dc_load_block(const double* __restrict__ A, int n, int k0, double* __restrict__ l) {
    for (int idx = threadIdx.x; idx < DC_NB * DC_NB; idx += DC_THREADS) {
        const int r = idx >> 6, c = idx & 63;
        l[r * DC_LD + c] = A[(size_t)(k0 + r) * n + k0 + c];
    }
}
// the factored block's lower triangle -> A
__device__ __forceinline__ void dc_store_lower(double* __restrict__ A, int n, int k0, const double* __restrict__ l) {
    for (int idx = threadIdx.x; idx < DC_NB * DC_NB; idx += DC_THREADS) {
        const int r = idx >> 6, c = idx & 63;
        if (c <= r) A[(size_t)(k0 + r) * n + k0 + c] = l[r * DC_LD + c];
    }
}

// the diagonal block of step 0 (the later ones are factored by dc_update_kernel one step ahead).  force_fail: PGO_DEBUG_BREAK_DENSE
__global__ __launch_bounds__(DC_THREADS) void dc_first_block_kernel(double* __restrict__ A, int n, int32_t* __restrict__ fail, int force_fail) {
    __shared__ double l[DC_NB * DC_LD];
    dc_load_block(A, n, 0, l);
    __syncthreads();
    const bool bad = dc_factor_block(DcTeam{}, l);
    dc_store_lower(A, n, 0, l);
    if (threadIdx.x == 0 && (bad || force_fail)) *fail = 1;
}

// Panel of step k: one workgroup per tile row i > k, one wavefront per 16 rows x of it.  The wavefront solves L_kk Y = (A_xk)^T by 16-wide block rows j: the products with
// the block rows solved before it on the MFMA — Y_m leaves the accumulator in the D layout (row lk + 4 reg, column lr), which IS the B layout of the next product's k = 4 kk + lk
// for reg = kk, so it never leaves the registers — then 16 substitution steps inside the 16 x 16 diagonal sub-block, the pivot row's value fetched with one cross-lane shuffle.
// Writes L_ik over A_ik and, k-major, into LT[64][ldu] for the update's coalesced operand loads.  The body is TILE_RSUB_FORWARD (pgo_tile_ops.hpp), which
// dcv_solve_kernel and the tile-sparse kernels expand too.
__global__ __launch_bounds__(DC_THREADS) void dc_panel_kernel(double* __restrict__ A, int n, int ldu, int k, double* __restrict__ LT) {
    __shared__ double l[DC_NB * DC_LD];
    const int k0 = k * DC_NB;
    dc_load_block(A, n, k0, l);
    __syncthreads();
    TILE_LANE;
    const int x0 = (k + 1 + (int)blockIdx.x) * DC_NB + wave * DC_SUB;      // < n: the grid has nt - k - 1 workgroups
    double* __restrict__ arow = A + (size_t)(x0 + lr) * n + k0;
    TILE_RSUB_FORWARD(l, arow[j * DC_SUB + lk + 4 * reg],
                      arow[j * DC_SUB + lk + 4 * reg] = r[reg];
                      LT[(size_t)(j * DC_SUB + lk + 4 * reg) * ldu + x0 + lr] = r[reg])
}

// Trailing update of step k: one workgroup per 64 x 64 tile (bi, bj), k < bj <= bi, 32 x 32 per wavefront as 2 x 2 MFMA tiles over K = 64, operands from the k-major
// copy of the panel.  The workgroup of tile (k + 1, k + 1) — dispatched first — keeps its tile in LDS, factors it there and writes the factor's lower triangle: the next
// step's diagonal block is never a launch of its own.
__global__ __launch_bounds__(DC_THREADS) void dc_update_kernel(double* __restrict__ A, int n, int ldu, int k, const double* __restrict__ LT, int32_t* __restrict__ fail) {
    __shared__ double a[DC_NB * DC_LD];
    const int bi = k + 1 + (int)blockIdx.y, bj = k + 1 + (int)blockIdx.x;      // < nt: the grid is (nt - k - 1)^2
    if (bj > bi) return;
    TILE_LANE;
    const int wr = wave >> 1, wc = wave & 1;
    const int i0 = bi * DC_NB + wr * 32, j0 = bj * DC_NB + wc * 32;
    const int k1 = (k + 1) * DC_NB;
    const bool ahead = bi == k + 1 && bj == k + 1;                 // this workgroup owns the next diagonal block
    if (!(bi == bj && wr == 0 && wc == 1)) {                       // (that quadrant lies above the diagonal)
        tile_d4 acc[2][2];
        double old[2][2][4];                                       // the tile's current values: all 16 loads in flight before the first store
        TILE_WALK_2X2(i0, j0, acc[s][u] = TILE_D4_ZERO, old[s][u][reg] = A[(size_t)i * n + j0 + u * 16 + lr])
        TILE_MFMA_2X2(acc, DC_NB / 4, const size_t row = (size_t)(kk * 4 + lk) * ldu, LT[row + i0 + lr], LT[row + i0 + 16 + lr], LT[row + j0 + lr], LT[row + j0 + 16 + lr])
        TILE_WALK_2X2(i0, j0, ,
                      const double v = old[s][u][reg] - acc[s][u][reg];
                      if (ahead) a[(i - k1) * DC_LD + (j - k1)] = v;      // (written to A once, as the factor)
                      else A[(size_t)i * n + j] = v)
    }
    if (!ahead) return;
    __syncthreads();
    const bool bad = dc_factor_block(DcTeam{}, a);
    dc_store_lower(A, n, k1, a);
    if (threadIdx.x == 0 && bad) *fail = 1;
}

// Forward sweep, step k: every workgroup solves L_kk y_k = w_k in LDS; the one of tile k writes y_k, the one of tile i > k takes L_ik y_k off its 64 rows of w
__global__ __launch_bounds__(DC_THREADS) void dc_forward_kernel(const double* __restrict__ A, int n, int k, double* __restrict__ w, double* __restrict__ yv) {
    __shared__ double l[DC_NB * DC_LD];
    __shared__ double v[DC_NB], y[DC_NB], part[DC_NB * 4];
    const int k0 = k * DC_NB, tid = threadIdx.x;
    const int i0 = (k + (int)blockIdx.x) * DC_NB;                  // < n: the grid has nt - k workgroups
    dc_load_block(A, n, k0, l);
    if (tid < DC_NB) v[tid] = w[k0 + tid];
    __syncthreads();
    dc_forward_block(DcTeam{}, l, v, y);
    if (blockIdx.x == 0) { if (tid < DC_NB) yv[k0 + tid] = y[tid]; return; }
    const int r = tid >> 2, q = tid & 3;
    const double* __restrict__ arow = A + (size_t)(i0 + r) * n + k0;
    double s = 0.0;
#pragma unroll
    for (int c = 16 * q; c < 16 * q + 16; ++c) s += arow[c] * y[c];
    part[r * 4 + q] = s;
    __syncthreads();
    if (tid < DC_NB) w[i0 + tid] -= dc_sum4(part[tid * 4], part[tid * 4 + 1], part[tid * 4 + 2], part[tid * 4 + 3]);
}

// Backward sweep, step k: every workgroup solves L_kk^T x_k = y_k; the one of tile k writes x_k (entries below n_out only), the one of tile j < k takes L_kj^T x_k off its
// 64 entries of y
__global__ __launch_bounds__(DC_THREADS) void dc_backward_kernel(const double* __restrict__ A, int n, int k, double* __restrict__ yv, double* __restrict__ x, int n_out) {
    __shared__ double l[DC_NB * DC_LD];
    __shared__ double v[DC_NB], xs[DC_NB], part[DC_NB * 4];
    const int k0 = k * DC_NB, tid = threadIdx.x;
    const int j0 = (int)blockIdx.x * DC_NB;                        // <= k0: the grid has k + 1 workgroups
    dc_load_block(A, n, k0, l);
    if (tid < DC_NB) v[tid] = yv[k0 + tid];
    __syncthreads();
    dc_backward_block(DcTeam{}, l, v, xs);
    if ((int)blockIdx.x == k) { if (tid < DC_NB && k0 + tid < n_out) x[k0 + tid] = xs[tid]; return; }
    const int c = tid & 63, q = tid >> 6;
    double s = 0.0;
#pragma unroll
    for (int r = 16 * q; r < 16 * q + 16; ++r) s += A[(size_t)(k0 + r) * n + j0 + c] * xs[r];
    part[c * 4 + q] = s;
    __syncthreads();
    if (tid < DC_NB) yv[j0 + tid] -= dc_sum4(part[tid * 4], part[tid * 4 + 1], part[tid * 4 + 2], part[tid * 4 + 3]);
}

// The reduced, damped block-CSR system (C.val, written by build_rows) -> the lower triangle of the zeroed dense matrix, and C.b -> w.  One thread per entry (a, c) of a block
// row: it walks the row's blocks in their stored order and ADDS (two edges between the same keyframes give two blocks at the same place), so no two threads meet at an
// address.  Rows and columns of keyframes outside the system (constant, unreferenced) and the padding up to n: identity, right-hand side 0.
__global__ __launch_bounds__(DC_THREADS) void dc_scatter_kernel(GraphDev G, CgDev C, double* __restrict__ A, int n, double* __restrict__ w) {
    const int64_t gid = (int64_t)blockIdx.x * DC_THREADS + threadIdx.x;
    const int64_t n6 = G.N * 6;
    if (gid >= G.N * 36) {
        const int64_t i = n6 + (gid - G.N * 36);
        if (i < n) { A[(size_t)i * n + i] = 1.0; w[i] = 0.0; }
        return;
    }
    const int64_t node = gid / 36;
    const int e = (int)(gid - node * 36), a = e / 6, c = e - a * 6;
    const size_t row = (size_t)node * 6 + a;
    if (!G.node_free[node]) {
        if (a == c) A[row * n + row] = 1.0;
        if (c == 0) w[row] = 0.0;
        return;
    }
    const int at = (a >> 1) * 12 + c * 2 + (a & 1);      // column-pair-major block layout
    for (int64_t b = G.bsr_rowptr[node]; b < G.bsr_rowptr[node + 1]; ++b) {
        const int32_t col = G.bsr_col[b];
        if (col > node || !G.node_free[col]) continue;
        A[row * n + (size_t)col * 6 + c] += C.val[(size_t)b * 36 + at];
    }
    if (c == 0) w[row] = C.b[row];
}

// ---- covariance blocks: forward substitution with many right-hand sides (the rows of W[m][n]), then one Gram product per requested pair

// Solve of step k: dc_panel_kernel's substitution (TILE_RSUB_FORWARD) on the tile rows of W instead of the tile rows of A below the diagonal: one workgroup per tile
// row that has started, one wavefront per 16 right-hand sides, Y = W_.k L_kk^-T over W_.k and, k-major, into YT[64][ldm].
__global__ __launch_bounds__(DC_THREADS) void dcv_solve_kernel(const double* __restrict__ A, int n, int k, double* __restrict__ W, int ldm, double* __restrict__ YT) {
    __shared__ double l[DC_NB * DC_LD];
    const int k0 = k * DC_NB;
    dc_load_block(A, n, k0, l);
    __syncthreads();
    TILE_LANE;
    const int x0 = (int)blockIdx.x * DC_NB + wave * DC_SUB;                // < m: the grid has at most m / 64 workgroups
    double* __restrict__ wrow = W + (size_t)(x0 + lr) * n + k0;
    TILE_RSUB_FORWARD(l, wrow[j * DC_SUB + lk + 4 * reg],
                      wrow[j * DC_SUB + lk + 4 * reg] = r[reg];
                      YT[(size_t)(j * DC_SUB + lk + 4 * reg) * ldm + x0 + lr] = r[reg])
}

// Update of step k: one workgroup per 64 x 64 tile (tile row R of W, block column bi > k), W_Ri -= Y_R L_ik^T, 32 x 32 per wavefront as 2 x 2 MFMA tiles over K = 64.
// A operand: the k-major copy of Y (coalesced); B operand: L_ik, loaded row by row into LDS (coalesced) and read from there column-wise.
__global__ __launch_bounds__(DC_THREADS) void dcv_update_kernel(const double* __restrict__ A, int n, int k, double* __restrict__ W, int ldm, const double* __restrict__ YT) {
    __shared__ double l[DC_NB * DC_LD];
    const int bi = k + 1 + (int)blockIdx.y;                                // < nt: the grid is rows x (nt - k - 1)
    const int k0 = k * DC_NB;
    for (int idx = threadIdx.x; idx < DC_NB * DC_NB; idx += DC_THREADS) {      // (through dc_load_block with a row and a column origin the kernel gets other instructions)
        const int r = idx >> 6, c = idx & 63;
        l[r * DC_LD + c] = A[(size_t)(bi * DC_NB + r) * n + k0 + c];
    }
    __syncthreads();
    TILE_LANE;
    const int wr = wave >> 1, wc = wave & 1;
    const int i0 = (int)blockIdx.x * DC_NB + wr * 32, j0 = wc * 32;        // rows of W (< m), columns inside the block column
    tile_d4 acc[2][2];
    double old[2][2][4];
    TILE_WALK_2X2(i0, j0, acc[s][u] = TILE_D4_ZERO, old[s][u][reg] = W[(size_t)i * n + bi * DC_NB + j0 + u * 16 + lr])
    TILE_MFMA_2X2(acc, DC_NB / 4, const size_t row = (size_t)(kk * 4 + lk) * ldm, YT[row + i0 + lr], YT[row + i0 + 16 + lr], l[(j0 + lr) * DC_LD + kk * 4 + lk], l[(j0 + 16 + lr) * DC_LD + kk * 4 + lk])
    TILE_WALK_2X2(i0, j0, , W[(size_t)i * n + bi * DC_NB + j0 + u * 16 + lr] = old[s][u][reg] - acc[s][u][reg])
}

// ---- the right-hand sides and the Gram products of pose and switch blocks (the algebra and the plan: pgo_dense_math.hpp)

// the right-hand sides into the zeroed W, one thread per row: a unit row's one, a switch row's -c_side / h (dc_param_rhs_row); a requested switch whose h cannot divide
// raises the failure flag
__global__ __launch_bounds__(DC_THREADS) void dcp_rhs_kernel(double* __restrict__ W, int n, int m, const int32_t* __restrict__ col, const int32_t* __restrict__ sw_node,
                                                             const double* __restrict__ sw_c, const double* __restrict__ sw_h, int32_t* __restrict__ fail) {
    const int r = (int)blockIdx.x * DC_THREADS + (int)threadIdx.x;
    if (r >= m) return;
    if (dc_param_rhs_row(W + (size_t)r * n, col[r], sw_node, sw_c, sw_h)) *fail = 1;
}

// One workgroup per requested pair (dc_param_gram): pr[5 pair ..]: the first rows of W of the two blocks, the Gram's first column, the sizes (d_a | d_b << 8), and the
// switch index when the pair is a switch with itself (1 / h is added), else -1.  Writes all 36 entries of the pair.
__global__ __launch_bounds__(DC_THREADS) void dcp_gram_kernel(const double* __restrict__ W, int n, const int32_t* __restrict__ pr, const double* __restrict__ sw_h, double* __restrict__ cov) {
    __shared__ double part[6 * DC_GRAM];
    const size_t pair = blockIdx.x;
    const int32_t* q = pr + 5 * pair;
    const int32_t s = q[4];
    dc_param_gram(DcTeam{}, W + (size_t)q[0] * n, q[3] & 255, W + (size_t)q[1] * n, q[3] >> 8, (size_t)n, n, q[2], s >= 0, s >= 0 ? 1.0 / sw_h[s] : 0.0, part, cov + 36 * pair);
}

// The undamped Schur complement of a matrix-free handle -> the zeroed dense matrix, from the normal blocks (DcMfPlan; dc_mf_diag_entry, dc_mf_offdiag_entry).  One thread per
// entry: the 36 of every keyframe's diagonal block (identity where it is not free), the padding's ones, the 36 of every lower-triangle off-diagonal block.  Each
// address has one writer.
struct DcMfDev { const int32_t* seg_ptr; const int32_t* seg_hi; const int32_t* seg_lo; const int32_t* ent; const int32_t* side_ptr; const int32_t* side; int64_t segments; };
__global__ __launch_bounds__(DC_THREADS) void dcm_scatter_kernel(int64_t N, const uint8_t* __restrict__ node_free, DcMfDev M, const double* __restrict__ Hd, const double* __restrict__ hoff_rel,
                                                                 const double* __restrict__ hoff_sw, const double* __restrict__ sw_c, const double* __restrict__ sw_h, double* __restrict__ A, int n) {
    const int64_t gid = (int64_t)blockIdx.x * DC_THREADS + threadIdx.x;
    const int64_t n36 = N * 36, pad = (int64_t)n - N * 6;
    if (gid < n36) {
        const int64_t node = gid / 36;
        const int e = (int)(gid - node * 36), a = e / 6, c = e - a * 6;
        const size_t row = (size_t)node * 6 + a;
        if (node_free[node]) A[row * n + (size_t)node * 6 + c] = dc_mf_diag_entry(Hd + (size_t)node * 36, M.side, M.side_ptr[node], M.side_ptr[node + 1], a, c, sw_c, sw_h);
        else if (a == c) A[row * n + row] = 1.0;
        return;
    }
    if (gid < n36 + pad) { const size_t i = (size_t)(N * 6 + (gid - n36)); A[i * n + i] = 1.0; return; }
    const int64_t t = gid - n36 - pad, s = t / 36;
    if (s >= M.segments) return;
    const int e = (int)(t - s * 36), a = e / 6, c = e - a * 6;
    A[((size_t)M.seg_hi[s] * 6 + a) * n + (size_t)M.seg_lo[s] * 6 + c] = dc_mf_offdiag_entry(M.ent, M.seg_ptr[s], M.seg_ptr[s + 1], a, c, hoff_rel, hoff_sw, sw_c, sw_h);
}

struct DcLaunch {
    double* A; int n, ldu; double* LT; int32_t* fail; int force_fail; double* w; double* yv; double* x; int n_out; hipStream_t st;
    int nt() const { return n / DC_NB; }
    void factor_first() { hipLaunchKernelGGL(dc_first_block_kernel, dim3(1), dim3(DC_THREADS), 0, st, A, n, fail, force_fail); }
    void panel(int k) { hipLaunchKernelGGL(dc_panel_kernel, dim3((unsigned)(nt() - k - 1)), dim3(DC_THREADS), 0, st, A, n, ldu, k, LT); }
    void update(int k) { hipLaunchKernelGGL(dc_update_kernel, dim3((unsigned)(nt() - k - 1), (unsigned)(nt() - k - 1)), dim3(DC_THREADS), 0, st, A, n, ldu, k, (const double*)LT, fail); }
    void forward(int k) { hipLaunchKernelGGL(dc_forward_kernel, dim3((unsigned)(nt() - k)), dim3(DC_THREADS), 0, st, (const double*)A, n, k, w, yv); }
    void backward(int k) { hipLaunchKernelGGL(dc_backward_kernel, dim3((unsigned)(k + 1)), dim3(DC_THREADS), 0, st, (const double*)A, n, k, yv, x, n_out); }
};
struct DcCovLaunch {
    const double* A; int n; double* W; int ldm; double* YT; hipStream_t st;
    int nt() const { return n / DC_NB; }
    void cov_solve(int k, int rows) { hipLaunchKernelGGL(dcv_solve_kernel, dim3((unsigned)rows), dim3(DC_THREADS), 0, st, A, n, k, W, ldm, YT); }
    void cov_update(int k, int rows) { hipLaunchKernelGGL(dcv_update_kernel, dim3((unsigned)rows, (unsigned)(nt() - k - 1)), dim3(DC_THREADS), 0, st, A, n, k, W, ldm, (const double*)YT); }
};

}  // namespace

size_t dense_scratch_doubles(int n) { return (size_t)DC_NB * (size_t)(n + 16); }

void launch_dense_factor(double* A, int n, double* scratch, int32_t* fail, bool force_fail, hipStream_t st) {
    DcLaunch D{A, n, n + 16, scratch, fail, force_fail ? 1 : 0, nullptr, nullptr, nullptr, 0, st};
    dc_factor_steps(n, D);
}
void launch_dense_solve(const double* A, int n, double* w, double* yv, double* x, int n_out, hipStream_t st) {
    DcLaunch D{const_cast<double*>(A), n, n + 16, nullptr, nullptr, 0, w, yv, x, n_out, st};
    dc_solve_steps(n, D);
}
void launch_dense_scatter(const GraphDev& G, const CgDev& C, double* A, int n, double* w, hipStream_t st) {
    const int64_t threads = G.N * 36 + ((int64_t)n - G.N * 6);
    hipLaunchKernelGGL(dc_scatter_kernel, dim3((unsigned)((threads + DC_THREADS - 1) / DC_THREADS)), dim3(DC_THREADS), 0, st, G, C, A, n, w);
}

// ---- covariance blocks of pose and switch parameters (pgo_pose_covariance, pgo_covariance, the two pgo_dense_spd_*covariance hooks).  work: dense_cov_doubles(n, Q.m,
// pairs) doubles — W, the k-major copy of a solved block column, the blocks; idx: dense_param_ints(Q.m, pairs, switches) — the rows' columns, five numbers per pair
// (dcp_gram_kernel), the switches' two nodes.  sw_c [12 per switch], sw_h: device arrays.
size_t dense_cov_doubles(int n, int m, int64_t n_pairs) { return (size_t)m * n + (size_t)DC_NB * (m + 16) + (size_t)36 * n_pairs; }
double* dense_cov_blocks(double* work, int n, int m) { return work + (size_t)m * n + (size_t)DC_NB * (m + 16); }
size_t dense_param_ints(int m, int64_t n_pairs, int64_t n_sw) { return (size_t)m + (size_t)5 * n_pairs + (size_t)2 * n_sw; }
int dense_param_upload(pgo_problem* p, const DcParamPlan& Q, int64_t n_sw, const int32_t* sw_node, std::vector<int32_t>& staging, int32_t* idx) {
    const size_t np = Q.row_a.size();
    staging.assign(Q.col.begin(), Q.col.end());
    for (size_t k = 0; k < np; ++k) for (int32_t v : {Q.row_a[k], Q.row_b[k], (int32_t)Q.gram_c0((int64_t)k), Q.dim_a[k] | (Q.dim_b[k] << 8), Q.self_switch[k]}) staging.push_back(v);
    staging.insert(staging.end(), sw_node, sw_node + 2 * n_sw);
    HIPCHK(p, hipMemcpyAsync(idx, staging.data(), staging.size() * sizeof(int32_t), hipMemcpyHostToDevice, p->st));      // (staging outlives the caller's next synchronize)
    return PGO_OK;
}
// the right-hand sides: needs no factor, so it runs ahead of the factorisation and shares its failure flag and its one synchronisation
int launch_dense_param_rhs(pgo_problem* p, int n, const DcParamPlan& Q, double* work, const int32_t* idx, const double* sw_c, const double* sw_h, int32_t* fail) {
    const int m = Q.m;
    const int64_t np = (int64_t)Q.row_a.size();
    HIPCHK(p, hipMemsetAsync(work, 0, (size_t)m * n * sizeof(double), p->st));
    hipLaunchKernelGGL(dcp_rhs_kernel, dim3((unsigned)((m + DC_THREADS - 1) / DC_THREADS)), dim3(DC_THREADS), 0, p->st, work, n, m, idx, idx + m + 5 * np, sw_c, sw_h, fail);
    return PGO_OK;
}
// the substitutions and the Gram products, on the factor in A
void launch_dense_param_covariance(pgo_problem* p, const double* A, int n, const DcParamPlan& Q, double* work, const int32_t* idx, const double* sw_h) {
    const int m = Q.m;
    const int64_t np = (int64_t)Q.row_a.size();
    DcCovLaunch D{A, n, work, m + 16, work + (size_t)m * n, p->st};
    dc_cov_steps(n, Q.mt, Q.start_tile.data(), true, D);
    hipLaunchKernelGGL(dcp_gram_kernel, dim3((unsigned)np), dim3(DC_THREADS), 0, p->st, (const double*)work, n, idx + m, sw_h, dense_cov_blocks(work, n, m));
}

// ---- the handle's side
bool dense_mode(const pgo_problem* p) { return p->opt.linear_solver == PGO_LINEAR_DENSE_CHOLESKY; }

int dense_allocate(pgo_problem* p) {
    DenseState& d = p->dense;
    d.n = (int)((p->N * 6 + DC_NB - 1) / DC_NB * DC_NB);
    if (d.n < DC_NB) d.n = DC_NB;
    HIPCHK(p, d.A.ensure((size_t)d.n * d.n)); HIPCHK(p, d.scratch.ensure(dense_scratch_doubles(d.n))); HIPCHK(p, d.vec.ensure((size_t)2 * d.n));
    d.built = true;
    return PGO_OK;
}
void dense_release(pgo_problem* p) {
    DenseState& d = p->dense;
    for (DBuf<double>* b : {&d.A, &d.scratch, &d.vec, &d.cov}) { if (b->p) (void)hipFree(b->p); b->p = nullptr; b->cap = 0; }
    if (d.cov_idx.p) { (void)hipFree(d.cov_idx.p); d.cov_idx.p = nullptr; d.cov_idx.cap = 0; }
    d.n = 0; d.built = false;
}

// One dense step on the system build_system has left in C.val / C.b: scatter + factor (timed as the system by lm_step), the failure flag, then the sweeps into C.x.
// *ok = false: a pivot was not positive (or NaN), nothing was solved.  *t_factored: the host clock between the two halves.
int dense_step(pgo_problem* p, bool* ok, double* t_factored) {
    DenseState& d = p->dense;
    if (!d.built || p->built_mf) { p->err = "dense Cholesky: the graph was not built for it"; return PGO_ERR_STATE; }
    const int n = d.n;
    int32_t* fail = p->d_flags.p + 4;
    HIPCHK(p, hipMemsetAsync(d.A.p, 0, (size_t)n * n * sizeof(double), p->st));
    HIPCHK(p, hipMemsetAsync(fail, 0, sizeof(int32_t), p->st));
    launch_dense_scatter(p->G, p->C, d.A.p, n, d.vec.p, p->st);
    launch_dense_factor(d.A.p, n, d.scratch.p, fail, debug_break_dense(), p->st);
    int32_t h = 0;
    HIPCHK(p, hipMemcpyAsync(&h, fail, sizeof(int32_t), hipMemcpyDeviceToHost, p->st));
    HIPCHK(p, hipStreamSynchronize(p->st));
    *t_factored = now_s();
    *ok = h == 0;
    if (!*ok) return PGO_OK;
    launch_dense_solve(d.A.p, n, d.vec.p, d.vec.p + n, p->C.x, (int)(p->N * 6), p->st);
    HIPCHK(p, hipStreamSynchronize(p->st));
    return PGO_OK;
}

// The blocks of pgo_pose_covariance and pgo_covariance on the linearisation solve_begin has left (ia, ib: the pairs whose keyframes are all free, n_pairs >= 1).  Block
// ids: a free keyframe, or N + the internal index of a switchable edge; sw_node: per switchable edge its two keyframes, -1 where one is constant.  On a graph with
// block-CSR values the matrix is the undamped reduced system (the damping is diag / (radius s^2): exactly zero at radius = +inf, in the pose rows and in the switches'
// Schur terms alike) in build_rows' values, scattered; the system build_rows writes is in the tangent coordinates themselves — the Jacobi scaling only shapes the
// damping — so there is no scaling to undo on the way out.  On a matrix-free graph it is assembled from the normal blocks (J1^T J2 per edge formed here, as
// pgo_get_normal_blocks does), the graph stays what it is.  *ok = false: a pivot failed or a requested switch's h cannot divide, out untouched.
int dense_param_covariance(pgo_problem* p, const std::vector<int32_t>& sw_node, int64_t n_pairs, const int32_t* ia, const int32_t* ib, double* out, bool* ok) {
    DenseState& d = p->dense;
    int rc;
    if (!d.built && (rc = dense_allocate(p)) != PGO_OK) return rc;      // (until the handle's next graph build)
    const int n = d.n;
    const int64_t Es = p->G.sw.E;
    const DcParamPlan Q(n, (int32_t)p->N, sw_node.data(), n_pairs, ia, ib);
    HIPCHK(p, d.cov.ensure(dense_cov_doubles(n, Q.m, n_pairs))); HIPCHK(p, d.cov_idx.ensure(dense_param_ints(Q.m, n_pairs, Es)));
    std::vector<int32_t> staging, mf_staging;
    DBuf<int32_t> d_mf;
    if ((rc = dense_param_upload(p, Q, Es, sw_node.data(), staging, d.cov_idx.p)) != PGO_OK) return rc;
    int32_t* fail = p->d_flags.p + 4;
    HIPCHK(p, hipMemsetAsync(fail, 0, sizeof(int32_t), p->st));
    if ((rc = launch_dense_param_rhs(p, n, Q, d.cov.p, d.cov_idx.p, p->L.c, p->L.hss, fail)) != PGO_OK) return rc;
    HIPCHK(p, hipMemsetAsync(d.A.p, 0, (size_t)n * n * sizeof(double), p->st));
    if (p->built_mf) {
        HIPCHK(p, p->d_Hoff.ensure((size_t)(p->G.rel.Epad + p->G.sw.Epad) * 36));
        p->L.Hoff = p->d_Hoff.p;
        launch_k2_offdiag(p->G, p->L, p->st);
        const DcMfPlan M(p->N, p->h_node_free.data(), p->rel.size(), p->rel.c1.data(), p->rel.c2.data(), p->swe.size(), p->swe.c1.data(), p->swe.c2.data());
        size_t at[6], total = 0;
        const std::vector<int32_t>* parts[6] = {&M.seg_ptr, &M.seg_hi, &M.seg_lo, &M.ent, &M.side_ptr, &M.side};
        for (int k = 0; k < 6; ++k) { at[k] = total; mf_staging.insert(mf_staging.end(), parts[k]->begin(), parts[k]->end()); total = mf_staging.size(); }
        HIPCHK(p, d_mf.upload(mf_staging, p->st));
        const DcMfDev Md{d_mf.p + at[0], d_mf.p + at[1], d_mf.p + at[2], d_mf.p + at[3], d_mf.p + at[4], d_mf.p + at[5], M.segments()};
        const int64_t threads = p->N * 36 + ((int64_t)n - p->N * 6) + M.segments() * 36;
        hipLaunchKernelGGL(dcm_scatter_kernel, dim3((unsigned)((threads + DC_THREADS - 1) / DC_THREADS)), dim3(DC_THREADS), 0, p->st, (int64_t)p->N, p->G.node_free, Md, (const double*)p->L.Hd,
                           (const double*)p->L.Hoff, (const double*)(p->L.Hoff + (size_t)p->G.rel.Epad * 36), (const double*)p->L.c, (const double*)p->L.hss, d.A.p, n);
    } else {
        launch_lm_diag(p->G, p->L, p->Sc, p->opt.min_lm_diagonal, p->opt.max_lm_diagonal, p->st);      // (finite numbers for build_rows' division, whatever the buffers held)
        launch_build_rows(p->G, p->L, p->Sc, p->C, std::numeric_limits<double>::infinity(), 1, nullptr, p->ScMf.a_inv, p->st);
        launch_dense_scatter(p->G, p->C, d.A.p, n, d.vec.p, p->st);
    }
    launch_dense_factor(d.A.p, n, d.scratch.p, fail, debug_break_dense(), p->st);
    int32_t h = 0;
    HIPCHK(p, hipMemcpyAsync(&h, fail, sizeof(int32_t), hipMemcpyDeviceToHost, p->st));
    HIPCHK(p, hipStreamSynchronize(p->st));      // (the staging vectors and the plan's device copy are done with their uploads here; d_mf is read by nothing launched later)
    *ok = h == 0;
    if (!*ok) return PGO_OK;
    launch_dense_param_covariance(p, d.A.p, n, Q, d.cov.p, d.cov_idx.p, p->L.hss);
    HIPCHK(p, hipMemcpyAsync(out, dense_cov_blocks(d.cov.p, n, Q.m), (size_t)36 * n_pairs * sizeof(double), hipMemcpyDeviceToHost, p->st));
    HIPCHK(p, hipStreamSynchronize(p->st));
    return PGO_OK;
}

}  // namespace pgo
