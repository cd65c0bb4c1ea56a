// pgo_tile_ops.hpp — the fp64 MFMA tile arithmetic (v_mfma_f64_16x16x4_f64) that kernels of both libraries share, each body written once: the dense Cholesky solver
// (pgo_dense.hip) and the coarse operator's Gauss-Jordan inverse (pgo_kernels.hip) of libpgo.so, and the tile-sparse Cholesky kernels (pgo_sparse_kernels.hpp) of
// libpgo_sparse.so.  The bodies are MACROS, not functions: the kernels' instruction sequences are pinned to those of the copies these bodies replaced
// (profiles/sparse_kernel_refactor_check.txt, profiles/tile_ops_refactor_check.txt), and a body that the compiler sees as a function — inlined, with functor arguments or
// without — is scheduled differently (profiles/sparse_kernel_refactor_times.txt).  A macro's expansion is the text the kernel had.  Every body expects `TILE_LANE;` in
// scope (lr, lk); its other operands are arguments.  `-ffp-contract=on`: keep every expression as it stands.  The spelling of an address expression in an argument
// decides the instructions too: (size_t)i * n + j0 + u * 16 + lr adds the column terms one by one in 64 bits, (size_t)i * n + j adds the walk's int j once.
//   TILE_RSUB_FORWARD                          X L_kk^T = R, a wavefront's 16 rows: dc_panel_kernel, dcv_solve_kernel; sc_panel_kernel, sc_pfwd_kernel
//   TILE_RSUB_BACKWARD                         X L_kk = R: sc_sel_ginv_kernel, sc_pbwd_kernel
//   TILE_ZERO_2X2, TILE_MFMA_2X2, TILE_WALK_2X2  a wavefront's 32 x 32 quadrant of a 64 x 64 x K product.  K = 64: dc_update_kernel, dcv_update_kernel; sc_update_kernel,
//                                              sc_sel_column_kernel, sc_sel_diag_kernel.  K = 32: gj_update_kernel, gj_step_kernel
//   TILE_ROW_PANEL_MFMA                        a wavefront's 16 rows of W times a tile of L, read by rows or by columns: sc_pfwd_kernel, sc_pbwd_kernel
// The comment above dc_panel_kernel (pgo_dense.hip) derives the operand maps and the summation order; the one above gj_block_inverse (pgo_kernels.hip) states the
// instruction's.  Deliberately not here: the Gauss-Jordan kernels' product P u of the pivot inverse with 16 couplings (two accumulators over K = 32, no quadrant),
// which only they use — GJ_PIVOT_TIMES_U, beside them in pgo_kernels.hip; and dcv_update_kernel's own loop that loads L_ik into LDS, which through dc_load_block with a
// row and a column origin gave that kernel other instructions.
#pragma once
#include <hip/hip_runtime.h>

#include "pgo_dense_math.hpp"

namespace pgo {

namespace {

typedef double tile_d4 __attribute__((ext_vector_type(4)));
#define TILE_D4_ZERO tile_d4{0.0, 0.0, 0.0, 0.0}

// a thread's place in its workgroup of four wavefronts: a lane (lr, lk) holds, of a 16 x 16 MFMA tile, the entries lk + 4 reg (reg = 0 .. 3) of line lr.  (As the
// members of a struct the same four values gave the sparse kernels other instructions.)
#define TILE_LANE const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lr = lane & 15, lk = lane >> 4

// X L^T = R for the wavefront's 16 rows, l = the lower triangular L in LDS (stride DC_LD): dc_panel_kernel's scheme.  The 16-wide block columns j from the first to the
// last: r[reg] = R_ENTRY — the lane's entry of R in column j * DC_SUB + lk + 4 * reg, an expression in j and reg —, minus the MFMA products with the block columns
// already solved (m = 0 .. j - 1), then the substitution inside the diagonal sub-block from its first column to its last, one __shfl per column; the remaining
// arguments: statements in j and reg that put r[reg] where the solved entry goes.
#define TILE_RSUB_FORWARD(l, R_ENTRY, ...)                                                                                                                    \
    tile_d4 Y[DC_NB / DC_SUB];                                                                                                                                \
    _Pragma("unroll") for (int j = 0; j < DC_NB / DC_SUB; ++j) {                                                                                            \
        double r[4];                                                                                                                                        \
        _Pragma("unroll") for (int reg = 0; reg < 4; ++reg) r[reg] = R_ENTRY;                                                                               \
        tile_d4 sub = {0.0, 0.0, 0.0, 0.0};                                                                                                                   \
        _Pragma("unroll") for (int m = 0; m < j; ++m)                                                                                                       \
            _Pragma("unroll") for (int kk = 0; kk < 4; ++kk)                                                                                                \
                sub = __builtin_amdgcn_mfma_f64_16x16x4f64(l[(j * DC_SUB + lr) * DC_LD + m * DC_SUB + 4 * kk + lk], Y[m][kk], sub, 0, 0, 0);          \
        _Pragma("unroll") for (int reg = 0; reg < 4; ++reg) r[reg] = r[reg] - sub[reg];                                                                     \
        _Pragma("unroll") for (int p = 0; p < DC_SUB; ++p) {                                                                                                \
            const double yp = __shfl(r[p >> 2], (p & 3) * 16 + lr) / l[(j * DC_SUB + p) * DC_LD + j * DC_SUB + p];                                       \
            _Pragma("unroll") for (int reg = 0; reg < 4; ++reg) {                                                                                           \
                const int q = lk + 4 * reg;                                                                                                              \
                const double lqp = l[(j * DC_SUB + (q > p ? q : p)) * DC_LD + j * DC_SUB + p];      /* (q <= p: the diagonal entry, unused) */              \
                r[reg] = q == p ? yp : (q > p ? r[reg] - lqp * yp : r[reg]);                                                                                \
            }                                                                                                                                               \
        }                                                                                                                                                   \
        _Pragma("unroll") for (int reg = 0; reg < 4; ++reg) {                                                                                               \
            Y[j][reg] = r[reg];                                                                                                                             \
            __VA_ARGS__;                                                                                                                                    \
        }                                                                                                                                                   \
    }

// X L = R: TILE_RSUB_FORWARD run backwards — the block columns from the last to the first, MFMA products with the block columns already solved (m = 3 .. j + 1),
// substitution inside the diagonal sub-block from its last column to its first.  Operand map: A[i][k] = L[16 m + k][16 j + i], B[k][n] = X[row n][16 m + k],
// D[i][n] = (X_m L_mj)[row n][16 j + i]; a lane holds row lr, columns lk + 4 reg.
#define TILE_RSUB_BACKWARD(l, R_ENTRY, ...)                                                                                                                   \
    tile_d4 Y[DC_NB / DC_SUB];                                                                                                                                \
    _Pragma("unroll") for (int j = DC_NB / DC_SUB - 1; j >= 0; --j) {                                                                                       \
        double r[4];                                                                                                                                        \
        _Pragma("unroll") for (int reg = 0; reg < 4; ++reg) r[reg] = R_ENTRY;                                                                               \
        tile_d4 sub = {0.0, 0.0, 0.0, 0.0};                                                                                                                   \
        _Pragma("unroll") for (int m = DC_NB / DC_SUB - 1; m > j; --m)                                                                                      \
            _Pragma("unroll") for (int kk = 0; kk < 4; ++kk)                                                                                                \
                sub = __builtin_amdgcn_mfma_f64_16x16x4f64(l[(m * DC_SUB + 4 * kk + lk) * DC_LD + j * DC_SUB + lr], Y[m][kk], sub, 0, 0, 0);          \
        _Pragma("unroll") for (int reg = 0; reg < 4; ++reg) r[reg] = r[reg] - sub[reg];                                                                     \
        _Pragma("unroll") for (int p = DC_SUB - 1; p >= 0; --p) {                                                                                           \
            const double gp = __shfl(r[p >> 2], (p & 3) * 16 + lr) / l[(j * DC_SUB + p) * DC_LD + j * DC_SUB + p];                                       \
            _Pragma("unroll") for (int reg = 0; reg < 4; ++reg) {                                                                                           \
                const int q = lk + 4 * reg;                                                                                                              \
                const double lpq = l[(j * DC_SUB + p) * DC_LD + j * DC_SUB + (q < p ? q : p)];      /* (q >= p: the diagonal entry, unused) */              \
                r[reg] = q == p ? gp : (q < p ? r[reg] - lpq * gp : r[reg]);                                                                                \
            }                                                                                                                                               \
        }                                                                                                                                                   \
        _Pragma("unroll") for (int reg = 0; reg < 4; ++reg) {                                                                                               \
            Y[j][reg] = r[reg];                                                                                                                             \
            __VA_ARGS__;                                                                                                                                    \
        }                                                                                                                                                   \
    }

// the 2 x 2 MFMA tiles of a wavefront's 32 x 32 quadrant: tile_d4 acc[2][2], acc[s][u] = rows 16 s .., columns 16 u .. of the quadrant
#define TILE_ZERO_2X2(acc)                                                                                                                                    \
    _Pragma("unroll") for (int s = 0; s < 2; ++s)                                                                                                           \
        _Pragma("unroll") for (int u = 0; u < 2; ++u) acc[s][u] = TILE_D4_ZERO;
// acc += A B over K = 4 STEPS (DC_NB / 4 steps for a 64-wide tile, GJ_NB / 4 for the Gauss-Jordan block).  Per step kk: STEP, a declaration of what the operand
// expressions share (the inner index (kk * 4 + lk), scaled as the caller's operands need it); A0, A1: the lane's entries of A in rows lr and 16 + lr of the quadrant;
// B0, B1: of B in columns lr and 16 + lr
#define TILE_MFMA_2X2(acc, STEPS, STEP, A0, A1, B0, B1)                                                                                                       \
    _Pragma("unroll") for (int kk = 0; kk < STEPS; ++kk) {                                                                                                  \
        STEP;                                                                                                                                               \
        const double a0 = A0, a1 = A1, b0 = B0, b1 = B1;                                                                                                    \
        acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);                                                                       \
        acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);                                                                       \
        acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);                                                                       \
        acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);                                                                       \
    }
// the lane's sixteen entries (i, j) of the quadrant at (i0, j0) of the tile: PER_TILE, statements in s and u (may be empty), then for reg = 0 .. 3 the statements
// that follow, in s, u, reg, i and j
#define TILE_WALK_2X2(i0, j0, PER_TILE, ...)                                                                                                                  \
    _Pragma("unroll") for (int s = 0; s < 2; ++s)                                                                                                           \
        _Pragma("unroll") for (int u = 0; u < 2; ++u) {                                                                                                     \
            PER_TILE;                                                                                                                                       \
            _Pragma("unroll") for (int reg = 0; reg < 4; ++reg) {                                                                                           \
                const int i = i0 + s * 16 + lk + 4 * reg, j = j0 + u * 16 + lr;                                                                       \
                __VA_ARGS__;                                                                                                                                \
            }                                                                                                                                               \
        }

// tile_d4 acc[4]: acc[jb] += (the wavefront's row w of W, 64 entries) x (the tile l in LDS, stride DC_LD), block column jb of the result.  BY_COLUMNS false: W L^T, the
// tile read by rows (the forward sweep, tile (k, j)); true: W L, by columns (the backward sweep, tile (i, k)).  Formed transposed, D^T = L W^T, so that the sums arrive
// in TILE_RSUB_*'s layout.
#define TILE_ROW_PANEL_MFMA(acc, l, w, BY_COLUMNS)                                                                                                            \
    _Pragma("unroll") for (int kk = 0; kk < DC_NB / 4; ++kk) {                                                                                              \
        const double b = w[kk * 4 + lk];                                                                                                                 \
        _Pragma("unroll") for (int jb = 0; jb < DC_NB / DC_SUB; ++jb)                                                                                       \
            acc[jb] = __builtin_amdgcn_mfma_f64_16x16x4f64(BY_COLUMNS ? l[(kk * 4 + lk) * DC_LD + jb * DC_SUB + lr] : l[(jb * DC_SUB + lr) * DC_LD + kk * 4 + lk], b, acc[jb], 0, 0, 0); \
    }

}  // namespace

}  // namespace pgo
