// pgo_sparse_kernels.hpp — the device side of pgo_sparse_chol_* (include/pgo_sparse.h), included by pgo_sparse.hip: the companion library stays one translation unit.
// The six kernels of pgo_dense.hip with the matrix addressed through an ScPlan (pgo_sparse_math.hpp): tile storage `tiles` x 4096 doubles, the plan's tables on the
// device as int32 (ScDev).  The arithmetic of the diagonal tile, the panel, the update and the two sweeps is that of dc_first_block_kernel, dc_panel_kernel,
// dc_update_kernel, dc_forward_kernel and dc_backward_kernel: the block routines of pgo_dense_math.hpp and the MFMA tile bodies of pgo_tile_ops.hpp, two headers of
// libpgo.so that both libraries include — the same operand maps (the comment above dc_panel_kernel), the same summation order; this library still links no libpgo.so.
// In natural order the results are the dense solver's as numbers.
//
// The bodies of pgo_tile_ops.hpp that the kernels here expand: the substitution with a diagonal tile (sc_panel_kernel, sc_pfwd_kernel; backwards in sc_sel_ginv_kernel,
// sc_pbwd_kernel), the 2 x 2 MFMA product over K = 64 with its zeroing and store walk (sc_update_kernel, sc_sel_column_kernel, sc_sel_diag_kernel), the 16 x 64
// row-panel product (sc_pfwd_kernel, sc_pbwd_kernel) and the lane decomposition.
//
// Nothing waits on another workgroup inside a launch, there are no atomics, every sum has a fixed order.  The update finds its target tile by ScPlan::find's binary
// search in row_col, in device code (sc_find): no per-step pair table.
//
// The selected inverse (sc_sel_inverses_kernel, sc_sel_ginv_kernel, sc_sel_column_kernel, sc_sel_diag_kernel, then sc_sel_gather_kernel for 6 x 6 blocks) has no
// counterpart in pgo_dense.hip: Takahashi's recurrence on the tiles of L into a second tile array, under the same rules.
//
// The columns of the inverse in number (sc_pcol_rhs_kernel, sc_pfwd_kernel, sc_pbwd_kernel, sc_pgather_kernel) are the tile-sparse counterpart of dcv_solve_kernel /
// dcv_update_kernel — right-hand sides as the rows of W, 64 per workgroup — in the pull form and for both sweeps: blocks outside the pattern of L.
#include "pgo_sparse_blocks.hpp"
#include "pgo_tile_ops.hpp"

namespace pgo {

namespace {

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
    TILE_LANE;
    const int e = (int)blockIdx.x;                                         // < |s_k|: the grid
    const int x0 = e * DC_NB + wave * DC_SUB;
    double* __restrict__ arow = T + (size_t)P.col_tile[P.col_ptr[k] + e] * SC_TILE + (size_t)(wave * DC_SUB + lr) * DC_NB;
    TILE_RSUB_FORWARD(l, arow[j * DC_SUB + lk + 4 * reg],
                    arow[j * DC_SUB + lk + 4 * reg] = r[reg];
                    LT[(size_t)(j * DC_SUB + lk + 4 * reg) * ldu + x0 + lr] = r[reg])
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
    TILE_LANE;
    const int wr = wave >> 1, wc = wave & 1;
    const int i0 = wr * 32, j0 = wc * 32;                                  // inside the tile
    const int ia = pa * DC_NB + i0, jb = pb * DC_NB + j0;                  // columns of the k-major copy
    const bool ahead = p == 0 && P.ahead[k] != 0;                          // this workgroup owns the next diagonal tile
    if (!(pa == pb && wr == 0 && wc == 1)) {                               // (that quadrant lies above the diagonal)
        tile_d4 acc[2][2];
        double old[2][2][4];
        TILE_WALK_2X2(i0, j0, acc[s][u] = TILE_D4_ZERO, old[s][u][reg] = t[i * DC_NB + j])
        TILE_MFMA_2X2(acc, DC_NB / 4, const size_t row = (size_t)(kk * 4 + lk) * ldu, LT[row + ia + lr], LT[row + ia + 16 + lr], LT[row + jb + lr], LT[row + jb + 16 + lr])
        TILE_WALK_2X2(i0, j0, ,
                    const double v = old[s][u][reg] - acc[s][u][reg];
                    if (ahead) a[i * DC_LD + j] = v;      // (written to the tile once, as the factor)
                    else t[i * DC_NB + j] = v)
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
    TILE_LANE;
    const int e = (int)blockIdx.x;                                         // < |s_k|: the grid
    const double* __restrict__ arow = T + (size_t)P.col_tile[P.col_ptr[k] + e] * SC_TILE + (size_t)(wave * DC_SUB + lr) * DC_NB;
    double* __restrict__ grow = G + (size_t)e * SC_TILE + (size_t)(wave * DC_SUB + lr) * DC_NB;
    TILE_RSUB_BACKWARD(l, arow[j * DC_SUB + lk + 4 * reg], grow[j * DC_SUB + lk + 4 * reg] = r[reg])
}

// column(k): one workgroup per position a; Z_{s[a],k} = - sum_b Z(s[a], s[b]) G_b.  2 x 2 MFMA tiles per wavefront over K = 64 (sc_update_kernel's layout), the
// accumulators carried in registers over b ascending.  The tile Z(s[a], s[b]) goes through LDS: stored as (s[a], s[b]) where a >= b, as (s[b], s[a]) — read transposed —
// where a < b; the stride of 65 makes both walks conflict-free.
__global__ __launch_bounds__(SC_THREADS) void sc_sel_column_kernel(double* __restrict__ Z, ScDev P, int k, const double* __restrict__ G) {
    __shared__ double z[DC_NB * DC_LD];
    const int a = (int)blockIdx.x;                                         // < |s_k|: the grid
    const int c0 = P.col_ptr[k], m = P.col_ptr[k + 1] - c0, ra = P.col_row[c0 + a];
    TILE_LANE;
    const int i0 = (wave >> 1) * 32, j0 = (wave & 1) * 32;                 // inside the tile
    tile_d4 acc[2][2];
    TILE_ZERO_2X2(acc)
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
        TILE_MFMA_2X2(acc, DC_NB / 4, const int kx = kk * 4 + lk, z[(i0 + lr) * si + kx * sk], z[(i0 + 16 + lr) * si + kx * sk], g[kx * DC_NB + j0 + lr], g[kx * DC_NB + j0 + 16 + lr])
    }
    double* __restrict__ t = Z + (size_t)P.col_tile[c0 + a] * SC_TILE;      // a tile of column k: none of those read above
    TILE_WALK_2X2(i0, j0, , t[i * DC_NB + j] = -acc[s][u][reg])
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
    TILE_LANE;
    const int i0 = (wave >> 1) * 32, j0 = (wave & 1) * 32;
    if (i0 == 0 && j0 == 32) return;                                       // (that quadrant lies above the diagonal)
    tile_d4 acc[2][2];
    TILE_ZERO_2X2(acc)
    for (int a = 0; a < m; ++a) {
        const double* __restrict__ g = G + (size_t)a * SC_TILE;
        const double* __restrict__ zt = Z + (size_t)P.col_tile[c0 + a] * SC_TILE;
        TILE_MFMA_2X2(acc, DC_NB / 4, const int kx = (kk * 4 + lk) * DC_NB, g[kx + i0 + lr], g[kx + i0 + 16 + lr], zt[kx + j0 + lr], zt[kx + j0 + 16 + lr])
    }
    double* t = Z + (size_t)(P.row_ptr[k + 1] - 1) * SC_TILE;              // the diagonal tile: none of those read above
    TILE_WALK_2X2(i0, j0, ,
                if (i >= j) {
                    const double v = t[i * DC_NB + j] - acc[s][u][reg];
                    t[i * DC_NB + j] = v;
                    t[j * DC_NB + i] = v;
                })
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

// one tile of pfwd's / pbwd's carried sum: once every thread of the workgroup is done with what l held, tile `id` of T into l, then acc += (the wavefront's rows of
// W in tile column w_col) x (the tile, by rows or by columns: TILE_ROW_PANEL_MFMA).  The caller walks its own list of tiles.
#define SC_PANEL_TILE(acc, id, w_col, BY_COLUMNS)                      \
    {                                                                  \
        __syncthreads();                                               \
        sc_load_tile(T + (size_t)(id) * SC_TILE, l);                   \
        __syncthreads();                                               \
        const double* __restrict__ wt = wrow + (size_t)(w_col) * DC_NB; \
        TILE_ROW_PANEL_MFMA(acc, l, wt, BY_COLUMNS)                      \
    }

// pfwd(k): one workgroup per started panel (the grid).  acc = sum_j W_pj L_kj^T over the stored tiles (k, j), first[p] <= j < k, ascending; W_pk - acc, then
// sc_panel_kernel's substitution with L_kk.
__global__ __launch_bounds__(SC_THREADS) void sc_pfwd_kernel(const double* __restrict__ T, ScDev P, int k, int nc, double* __restrict__ W, const int32_t* __restrict__ first) {
    __shared__ double l[DC_NB * DC_LD];
    TILE_LANE;
    const int p = (int)blockIdx.x, fp = first[p];
    double* __restrict__ wrow = W + ((size_t)p * DC_NB + wave * DC_SUB + lr) * nc;
    const int diag = P.row_ptr[k + 1] - 1;
    tile_d4 acc[DC_NB / DC_SUB];
#pragma unroll
    for (int jb = 0; jb < DC_NB / DC_SUB; ++jb) acc[jb] = tile_d4{0.0, 0.0, 0.0, 0.0};
    for (int id = P.row_ptr[k]; id < diag; ++id) {
        const int j = P.row_col[id];
        if (j < fp) continue;                                              // (the same for every thread of the workgroup) W_pj is all zero
        SC_PANEL_TILE(acc, id, j, false)
    }
    __syncthreads();
    sc_load_tile(T + (size_t)diag * SC_TILE, l);
    __syncthreads();
    double* __restrict__ arow = wrow + (size_t)k * DC_NB;
    TILE_RSUB_FORWARD(l, arow[j * DC_SUB + lk + 4 * reg] - acc[j][reg], arow[j * DC_SUB + lk + 4 * reg] = r[reg])
}

// pbwd(k): one workgroup per panel (the grid).  acc = sum_{i in s_k} W_pi L_ik, i ascending; W_pk - acc, then sc_sel_ginv_kernel's substitution with L_kk.
__global__ __launch_bounds__(SC_THREADS) void sc_pbwd_kernel(const double* __restrict__ T, ScDev P, int k, int nc, double* __restrict__ W) {
    __shared__ double l[DC_NB * DC_LD];
    TILE_LANE;
    double* __restrict__ wrow = W + ((size_t)blockIdx.x * DC_NB + wave * DC_SUB + lr) * nc;
    tile_d4 acc[DC_NB / DC_SUB];
#pragma unroll
    for (int jb = 0; jb < DC_NB / DC_SUB; ++jb) acc[jb] = tile_d4{0.0, 0.0, 0.0, 0.0};
    for (int e = P.col_ptr[k]; e < P.col_ptr[k + 1]; ++e) SC_PANEL_TILE(acc, P.col_tile[e], P.col_row[e], true)
    __syncthreads();
    sc_load_tile(T + (size_t)(P.row_ptr[k + 1] - 1) * SC_TILE, l);
    __syncthreads();
    double* __restrict__ arow = wrow + (size_t)k * DC_NB;
    TILE_RSUB_BACKWARD(l, arow[j * DC_SUB + lk + 4 * reg] - acc[j][reg], arow[j * DC_SUB + lk + 4 * reg] = r[reg])
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

}  // namespace

}  // namespace pgo
