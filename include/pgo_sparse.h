/* pgo_sparse.h — C-ABI of libpgo_sparse.so: a tile-sparse exact Cholesky factorisation on the GPU (gfx950, fp64) for pose-graph systems above
 * PGO_DENSE_MAX_KEYFRAMES, covariance blocks from it, and the exact Levenberg-Marquardt step and solve on it (pgo_sparse_lm_*, further down).  A companion of libpgo.so, not a part of it: it links no libpgo.so, takes no pgo_problem and has no
 * option in pgo_options.  A caller carries a handle's system across with pgo_get_normal_blocks (every handle has it, matrix-free ones too) and
 * pgo_sparse_reduce_normal_blocks below.  Error codes are pgo.h's PGO_ERR_*.
 *
 * The matrix: n = 6 n_nodes rows padded to a multiple of 64, the keyframes in a permuted order (natural or reverse Cuthill-McKee), identity on the rows of
 * keyframes outside the system and on the padding; only the 64 x 64 tiles of the lower triangle in which the factor L can be non-zero are stored (tile-level
 * symbolic Cholesky).  With nt = n / 64 tile columns and s_k the tile rows below the diagonal of column k of L:
 *
 *   launches of one factorisation:  1 (diagonal tile 0) + per column k < nt - 1: panel (|s_k| workgroups) + update (|s_k| (|s_k| + 1) / 2 workgroups), and one
 *                                   more for the diagonal tile k + 1 when k + 1 is not in s_k; an empty s_k: that one alone.  (info8[5])
 *   launches of one pair of sweeps: 2 nt, whatever the number of right-hand sides: a workgroup handles one right-hand side, grid.y = n_rhs.  (info8[6])
 *
 * Nothing waits on another workgroup inside a launch, there are no atomics, every sum has a fixed order: two calls give the same bits.  In natural order the
 * numbers are those of pgo_dense_spd_solve on the same matrix.  All arrays are host arrays; every call returns after its work is done.
 * device_id: a HIP device, or -1 for the current one (pgo_options.device_id's convention); an object stays on the device it was created on. */
#ifndef PGO_SPARSE_H
#define PGO_SPARSE_H
#include <stdint.h>

#include "pgo.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PGO_SPARSE_MAX_RHS 65535      /* right-hand sides of one pgo_sparse_chol_solve: the sweeps put them on grid.y */
#define PGO_SPARSE_MAX_GROUPS 64      /* row groups of one pgo_sparse_chol_inverse_blocks */

/* sc_plan_graph's `ordering` */
enum { PGO_SPARSE_ORDER_AUTO = -1, PGO_SPARSE_ORDER_NATURAL = 0, PGO_SPARSE_ORDER_RCM = 1 };

typedef struct pgo_sparse_chol pgo_sparse_chol;

/* Solves a x = b for the symmetric positive definite n x n row-major matrix `a` with the tile-sparse kernels; row i at position pos[i] (a permutation of
 * 0 .. n - 1; NULL: where it is).  The tile pattern is that of the exact non-zeros of the lower triangle.  info8 (may be NULL): nt, tiles of the matrix,
 * tiles of L, 0, bytes of the tile storage, launches of one factorisation, of one pair of sweeps, tile updates.  The factor and the sweeps run `launches`
 * (>= 1) times between HIP events; *avg_ms (may be NULL): their average.  Launches per run: info8[5] + info8[6].
 * PGO_ERR_NUMERIC: a pivot was not > 0 (or NaN); x is left alone. */
int pgo_sparse_spd_solve(int32_t device_id, int32_t n, const double* a, const double* b, const int32_t* pos, double* x, int64_t* info8, int32_t launches, double* avg_ms);

/* Symbolic phase.  n_nodes keyframes; in_system[i] = 0: a constant or unreferenced keyframe (identity rows).  The n_pairs off-diagonal blocks of the system:
 * pair_hi[k], pair_lo[k] — two distinct keyframes of the system (any of the two may be the higher), every pair once, else PGO_ERR_INVALID_ARG.
 * ordering: PGO_SPARSE_ORDER_*.  Allocates the plan's device tables, the tile storage and the panel scratch on device_id.  No launch. */
int pgo_sparse_chol_create(int32_t device_id, int64_t n_nodes, const uint8_t* in_system, int64_t n_pairs, const int32_t* pair_hi, const int32_t* pair_lo, int32_t ordering, pgo_sparse_chol** out);
void pgo_sparse_chol_destroy(pgo_sparse_chol* h);

/* info8: as pgo_sparse_spd_solve's, the ordering used (0 natural, 1 reverse Cuthill-McKee) in slot 3.  order (may be NULL) [n_nodes]: the keyframe at every
 * position.  No launch. */
int pgo_sparse_chol_info(const pgo_sparse_chol* h, int64_t* info8, int32_t* order);

/* Numeric phase.  diag [n_nodes][36]: the diagonal blocks, row-major (those of keyframes outside the system are not read); pair_blocks [n_pairs][36]: the
 * block of pair k, rows of pair_hi[k], columns of pair_lo[k].  Launches: 1 (fill: pure copies into the zeroed tiles) + info8[5].
 * PGO_ERR_NUMERIC: a pivot was not > 0 (or NaN); the object has no factor then and takes another pgo_sparse_chol_factor. */
int pgo_sparse_chol_factor(pgo_sparse_chol* h, const double* diag, const double* pair_blocks);

/* X = A^-1 B for n_rhs right-hand sides, 1 <= n_rhs <= PGO_SPARSE_MAX_RHS; rows of B and X: 6 n_nodes doubles in the caller's keyframe order.  Entries of
 * keyframes outside the system are not read and come back exactly 0.  Launches: info8[6] = 2 nt.  Right-hand side r gets the bits it gets alone. */
int pgo_sparse_chol_solve(pgo_sparse_chol* h, int64_t n_rhs, const double* B, double* X);

/* Blocks of the inverse between sparse rows.  n_groups (1 .. PGO_SPARSE_MAX_GROUPS) groups of 1 or 6 rows: group g = rows group_ptr[g] .. group_ptr[g + 1] - 1;
 * row r = entries row_ptr[r] .. row_ptr[r + 1] - 1 of (col, val), col ascending, over the 6 n_nodes coordinates of the caller's keyframe order, on keyframes
 * of the system only.  out[36 k] = V_ga[k] A^-1 V_gb[k]^T, a d_a x d_b block row-major in the leading entries of its 36, the rest 0 (pgo_covariance's
 * layout).  Launches: 1 (the right-hand sides P v, copies) + nt - k0 (forward sweep only, all rows at once, from the first tile k0 that holds a non-zero
 * of any row: the skipped steps would write +0) + 1 (Gram products, dc_param_gram_block).  out of (b, a) is the exact transpose of out of (a, b).
 * For a handful of blocks: one workgroup per right-hand side per tile. */
int pgo_sparse_chol_inverse_blocks(pgo_sparse_chol* h, int64_t n_groups, const int64_t* group_ptr, const int64_t* row_ptr, const int32_t* col, const double* val,
                                   int64_t n_pairs, const int32_t* ga, const int32_t* gb, double* out);

/* The selected inverse: every entry of A^-1 that lies in the tile pattern of L — all diagonal blocks and the block of every pair given to pgo_sparse_chol_create —
 * by Takahashi's recurrence on the factor's tiles, one backward pass over the block columns (sc_selinv_steps).  For many blocks: every keyframe's marginal covariance,
 * every edge's joint covariance; no right-hand sides, no dense array.
 *   launches: 1 (L_kk^-T L_kk^-1 of every diagonal tile, nt workgroups: it reads L alone) + per column k with a non-empty s_k three, a chain: G = L_sk L_kk^-1
 *             (|s_k| workgroups), Z_sk = -Z_ss G (|s_k| workgroups), Z_kk -= G^T Z_sk (1 workgroup): info4[0].  Tile products (64 x 64 x 64, fp64 MFMA):
 *             |s_k|^2 + |s_k| per column, info4[1].
 *   memory:   a second tile array of info8[4] bytes (info4[2]), allocated by the first call and kept; G lives in the panel scratch.  The factor is only read:
 *             pgo_sparse_chol_solve and _inverse_blocks give afterwards the bits they gave before.
 * PGO_ERR_STATE: no factor.  A later pgo_sparse_chol_factor, successful or not, invalidates the selected inverse. */
int pgo_sparse_chol_selected_inverse(pgo_sparse_chol* h);
/* info4: launches of one pgo_sparse_chol_selected_inverse, its tile products, bytes of its tile array, 1 if a selected inverse of the present factor exists else 0.
 * No launch. */
int pgo_sparse_chol_selected_info(const pgo_sparse_chol* h, int64_t* info4);
/* Blocks of A^-1 from the selected inverse: out[36 k] = the 6 x 6 block, row-major, with the rows of keyframe node_a[k] and the columns of keyframe node_b[k] (the
 * caller's keyframe order; node_a[k] = node_b[k]: a marginal).  One launch, one thread per entry.  out of (b, a) is the exact transpose of out of (a, b), a diagonal
 * block is exactly symmetric.  A pair with a keyframe outside the system: a zero block (pgo_covariance's rule for constant keyframes).  A block of which any tile is
 * not in the pattern — two keyframes that share no block of the system and lie in tiles the factor does not fill — is reported, not guessed: zeros and
 * in_pattern[k] = 0 (else 1); with in_pattern = NULL it is PGO_ERR_INVALID_ARG, the pair named in the error text, and out is left alone.
 * PGO_ERR_STATE: no selected inverse of the present factor. */
int pgo_sparse_chol_selected_blocks(pgo_sparse_chol* h, int64_t n_blocks, const int32_t* node_a, const int32_t* node_b, double* out /*[n_blocks][36]*/, uint8_t* in_pattern /*[n_blocks], may be NULL*/);

/* Blocks of A^-1 between ANY keyframes, in number — the blocks outside the pattern of L, which the selected inverse has not: the cross-covariance of two keyframes
 * that share no edge yet (a loop-closure candidate).  col_node [n_cols]: distinct keyframes; out[36 k] = the 6 x 6 block, row-major, with the rows of keyframe
 * row_node[k] and the columns of keyframe col_node[col_index[k]].  The six unit columns of every column keyframe that a block asks for are solved by both sweeps as
 * the ROWS of a workspace W [m_pad][nc], in ascending position, 64 rows (a panel) per workgroup, the 64 x 64 x 64 tile products on the fp64 MFMA (sc_panel_steps):
 *   launches: per chunk 1 (the unit entries) + nt - k0 (forward, from the first tile k0 that holds a one) + nt - k_stop (backward, down to the lowest tile that holds
 *             a requested row) + 1 (gather): info4[0] of pgo_sparse_chol_columns_info; tile products: info4[1].
 *   memory:   W, at most the workspace limit (PGO_SPARSE_WORKSPACE_BYTES unless set): more columns than fit are served in chunks of whole keyframes, one after the
 *             other (info4[3]); allocated by the first call, grown on demand (info4[2]: bytes of the largest chunk of the last call), freed by _destroy.
 * A right-hand side gets the bits it gets alone, whatever the batch, the chunks and the rows asked for; no atomics, every sum in a fixed order.  The factor is only
 * read: pgo_sparse_chol_solve, _inverse_blocks and the selected inverse give afterwards the bits they gave before.  A block with a keyframe outside the system, as
 * row or as column: zeros.  The block of (b, a) through column a and that of (a, b) through column b are two computations: ask one and transpose it.
 * PGO_ERR_STATE: no factor.  PGO_ERR_INVALID_ARG, out left alone: a keyframe out of range, col_node not distinct, col_index out of range. */
#define PGO_SPARSE_WORKSPACE_BYTES ((int64_t)1 << 30)
int pgo_sparse_chol_inverse_columns(pgo_sparse_chol* h, int64_t n_cols, const int32_t* col_node, int64_t n_blocks, const int32_t* row_node, const int32_t* col_index, double* out /*[n_blocks][36]*/);
/* of the last pgo_sparse_chol_inverse_columns: launches, tile products, workspace bytes, chunks.  No launch. */
int pgo_sparse_chol_columns_info(const pgo_sparse_chol* h, int64_t* info4);
/* the most W may take from the next pgo_sparse_chol_inverse_columns on; at least one panel, 64 rows of 64 nt doubles, else PGO_ERR_INVALID_ARG */
int pgo_sparse_chol_set_workspace_limit(pgo_sparse_chol* h, int64_t bytes);

/* Host only: the undamped Schur complement S of a handle's last linearisation as blocks, from pgo_get_normal_blocks' arrays (diag [n_nodes][36], offdiag
 * [n_rel + n_sw][36]: J1^T J2 per edge, relative-pose then switchable, internal order; sw_c [n_sw][12]; sw_hss [n_sw]), the edges' endpoints in the same
 * order and node_free [n_nodes] (0: constant).  Per free keyframe H_ii - sum c c^T / h over its switch sides; per pair of free keyframes the sum in edge order
 * of J1^T J2 (transposed where c1 is the lower keyframe) minus c_hi c_lo^T / h for switchable edges.  Writes *n_pairs (<= n_rel + n_sw: the room pair_hi,
 * pair_lo and s_blocks [.][36] must have), pairs sorted by (higher, lower) keyframe, pair_hi > pair_lo; s_diag [n_nodes][36], zero where not free. */
int pgo_sparse_reduce_normal_blocks(int64_t n_nodes, const uint8_t* node_free, const double* diag, const double* offdiag, const double* sw_c, const double* sw_hss,
                                    int64_t n_rel, const int32_t* rel_c1, const int32_t* rel_c2, int64_t n_sw, const int32_t* swe_c1, const int32_t* swe_c2,
                                    int64_t* n_pairs, int32_t* pair_hi, int32_t* pair_lo, double* s_diag, double* s_blocks);

/* HIP-event milliseconds of the launches of the object's last pgo_sparse_chol_factor (fill included), _solve, _inverse_blocks, _selected_inverse, _selected_blocks or _inverse_columns */
double pgo_sparse_chol_last_ms(const pgo_sparse_chol* h);

/* ---- The exact Levenberg-Marquardt step and solve on the factor: Ceres' trust-region solve with every step the backward-stable solution of its system — what
 * PGO_LINEAR_DENSE_CHOLESKY gives up to PGO_DENSE_MAX_KEYFRAMES — for graphs of any size, beside the library: the linearisation comes through the hooks every handle has
 * (pgo_evaluate, pgo_get_normal_blocks, pgo_manifold_plus), the controller's decisions are csrc/pgo_lm.hpp's, the linear algebra of every step runs on the device here.
 * There is no option of pgo_options for it.
 *
 * One LM system (csrc/pgo_sparse_lm_math.hpp has the arithmetic per entry, shared by the kernels and a serial host instantiation):
 *   S_j = 1 / (1 + sqrt(H_jj)) per column, from the diagonals of `diag` (pose columns, before the switch elimination) and `sw_hss`, fixed at iteration 0;
 *   lambda_j = clamp(S_j^2 H_jj, min_lm_diagonal, max_lm_diagonal) / (radius S_j^2);   a_e = 1 / (h_e + lambda_e);
 *   (H_pp + diag(lambda_p) - sum_e c_e a_e c_e^T) dp = -(g_p - sum_e c_e a_e g_s,e);   ds_e = -a_e (g_s,e + c_e^T dp);
 *   model_cost_change = -d^T (g + H d / 2) with the full undamped H.
 * The damped Schur complement is written straight into the factor's zeroed tiles, each entry once as a sum in internal edge order; no atomics, every sum in a fixed
 * order: two calls give the same bits. */
typedef struct pgo_sparse_lm pgo_sparse_lm;

/* The step plan of a graph on `chol` (it must outlive the object, and both are used from one thread at a time).  node_free [n_nodes]: 0 for a constant keyframe; the
 * keyframes of the system are those with node_free != 0 that pgo_sparse_chol_create took with in_system != 0.  The edges in internal order — relative-pose in add order,
 * then switchable: the order of pgo_get_normal_blocks' offdiag.  Several edges may lie on one pair of keyframes, in either direction; an edge side on a keyframe outside
 * the system drops out, a switch with both endpoints outside keeps its pivot alone.  PGO_ERR_INVALID_ARG (text: pgo_sparse_last_error(NULL)): n_nodes is not the
 * factor's, a keyframe out of range, an edge from a keyframe to itself, a free endpoint that the factor keeps outside the system, or two keyframes of the system joined
 * by an edge that are no pair of the factor's pair list.  No launch. */
int pgo_sparse_lm_create(pgo_sparse_chol* chol, int64_t n_nodes, const uint8_t* node_free, int64_t n_rel, const int32_t* rel_c1, const int32_t* rel_c2,
                         int64_t n_sw, const int32_t* swe_c1, const int32_t* swe_c2, pgo_sparse_lm** out);
void pgo_sparse_lm_destroy(pgo_sparse_lm* lm);

/* The Jacobi scale S from a linearisation's diag [n_nodes][36] and sw_hss [n_sw]: at iteration 0 only.  diag = NULL: no scaling, S = 1 (pgo_options.jacobi_scaling = 0). */
int pgo_sparse_lm_set_scale(pgo_sparse_lm* lm, const double* diag, const double* sw_hss);

/* One exact LM step from pgo_get_normal_blocks' host arrays as they come: one upload, the launches — damping, fill, right-hand side, 1 + 1 + 1; the factor, info8[5];
 * the sweeps, info8[6]; back-substitution, model, its reduction, 1 + 1 + 1 — and one download.  delta_pose [6 n_nodes] in the caller's keyframe order, exactly 0 for a
 * keyframe outside the system; delta_sw [n_sw] per switchable edge; out3: model_cost_change, the tangent norm |d| (pose and switch entries), HIP-event milliseconds of
 * the factor.  PGO_ERR_NUMERIC: a pivot of the factor or a damped switch pivot is not > 0 (or NaN) — nothing but out3[2] is written, and the object takes the next step.
 * PGO_ERR_STATE: no scale.  The factor in `chol` is the damped system's afterwards: its covariance calls want a new pgo_sparse_chol_factor.
 * Error texts: pgo_sparse_last_error(chol). */
int pgo_sparse_lm_step(pgo_sparse_lm* lm, const double* diag, const double* grad, const double* offdiag, const double* sw_c, const double* sw_hss, const double* sw_gs,
                       double radius, double min_lm_diagonal, double max_lm_diagonal, double* delta_pose, double* delta_sw, double* out3);
/* HIP-event milliseconds of the last pgo_sparse_lm_step: upload, damping + fill + right-hand side, factor, sweeps, back-substitution + model, download.  No launch. */
int pgo_sparse_lm_last_times(const pgo_sparse_lm* lm, double* ms6);

/* pgo_evaluate, pgo_get_normal_blocks and pgo_manifold_plus without the handle; `user` is handed through.  A return other than 0 ends the solve with that code. */
typedef struct pgo_sparse_lm_callbacks {
    int (*evaluate)(void* user, const double* quat_xyzw, const double* t, const double* sw, int64_t n_nodes, int64_t n_switch, double* cost, double* residuals, double* gradient);
    int (*normal_blocks)(void* user, double* diag, double* grad, double* offdiag, double* sw_c, double* sw_hss, double* sw_gs);
    int (*manifold_plus)(void* user, int64_t n, const double* quat_xyzw, const double* t, const double* delta, double* quat_out, double* t_out);      /* t, t_out may be NULL */
} pgo_sparse_lm_callbacks;

/* The whole solve = pgo_solve with every step exact: lm_begin, lm_pre_step, lm_step_outcome, lm_outcome_stop and lm_finish_step of csrc/pgo_lm.hpp around
 * pgo_sparse_lm_step.  quat [4 n_nodes], t [3 n_nodes], sw [n_switch] hold the start and receive the result; swe_index [n_sw]: the switch index of every switchable
 * edge (NULL: edge e uses switch e).  Per iteration: the step; the candidate Plus(x, dp) through the callback and sw + ds, evaluated for its cost alone; an accepted
 * step is linearised again (evaluate with a gradient, then normal_blocks).  A failed factorisation is an invalid step (PGO_STEP_INVALID_FACTORIZATION) and the radius
 * halves: the dense solver's rule; the point's blocks are then fetched again (evaluate with a gradient, normal_blocks: a handle gives the numbers it gave before).  There is no pause plan — every step is exact.  The controller's step norm and x_norm are the handle's: ambient, 4 + 3 numbers per
 * keyframe of the system and one per switchable edge's switch.  `summary` is filled as the handle's dense solve fills it: preconditioner = PGO_PRECOND_DIRECT, zero CG
 * counts, seconds_system = the factor's HIP-event time.  The options read: max_num_iterations, jacobi_scaling, max_num_consecutive_invalid_steps, the trust-region
 * radii, min_relative_decrease, the LM diagonal's clamps and the three tolerances.  On PGO_FAILURE, and on any error return, the arrays are left unmodified. */
int pgo_sparse_lm_solve(pgo_sparse_lm* lm, const pgo_sparse_lm_callbacks* callbacks, void* user, int64_t n_switch, const int32_t* swe_index, double* quat_xyzw, double* t, double* sw,
                        const pgo_options* options, pgo_summary* summary);

/* ---- A pose graph that linearises itself: relative-pose, switchable and regulariser blocks with their own kernels in this library, so that the exact solve above needs no
 * pgo_problem — and the one place where yaw/pitch/roll-weighted edges (the reference's FourDOFError and FourDOFErrorWithSwitchingConstraints, src/CeresResidues.h:252-422) run
 * on the device.  It takes no pgo_problem and links no libpgo.so.  Conventions, residual order, internal edge order (relative-pose in add order, then switchable) and the tangent
 * layout are include/pgo.h's; robust blocks follow Problem::Evaluate with apply_loss_function = true, as on a handle.
 *
 * Edge kinds.  ypr_gains = NULL, or an edge's three gains (0, 0, 0): a SixDOFError edge, r6 = w [dt ; 2 dq.vec].  Three gains > 0: a yaw/pitch/roll edge,
 * r6 = w [dt ; g_y yaw ; g_p pitch ; g_r roll] in degrees (the reference's own gains: 4, 10, 10); pitch error +-90 degrees is the Euler singularity of the reference's functor and
 * is not handled: the block turns non-finite.  A switchable edge ignores the weight and multiplies all seven rows by s, as the reference does: r = [s r6 ; s (1 - s)].
 *
 * One linearisation = pgo_sparse_graph_evaluate with a gradient: a block kernel (one thread per residual block), a one-workgroup cost reduction, a node kernel (one thread per
 * keyframe over its incident list in list order: internal edge order, regularisers last).  A cost-only evaluation: the block kernel without Jacobians and the reduction.  No
 * atomics, one writer per address, nothing waits on another workgroup, every address from the tables of _finalize: two calls give the same bits.  All arrays are host arrays.
 *
 * PGO_ERR_INVALID_ARG — nothing is added, nothing is launched, the text in pgo_sparse_last_error(NULL): a keyframe out of range, an edge from a keyframe to itself, gains that
 * are neither all zero nor all > 0 and finite, an unknown loss, a loss_a that is not finite or <= 0 on a non-trivial loss, a switch index used twice, a non-finite measurement.
 * PGO_ERR_STATE: blocks added after _finalize, an evaluation before it, _normal_blocks / _jacobian_blocks before an evaluation with a gradient. */
typedef struct pgo_sparse_graph pgo_sparse_graph;

int pgo_sparse_graph_create(int64_t n_nodes, int32_t device_id, pgo_sparse_graph** out);
void pgo_sparse_graph_destroy(pgo_sparse_graph* g);
/* c1_T_c2: n x 16 doubles (column-major Matrix4d); weight [n]; ypr_gains [3 n] (yaw, pitch, roll per edge) or NULL; loss: PGO_LOSS_*, loss_a its parameter */
int pgo_sparse_graph_add_relpose_edges(pgo_sparse_graph* g, int64_t n, const int32_t* c1, const int32_t* c2, const double* c1_T_c2, const double* weight, const double* ypr_gains, int32_t loss,
                                       double loss_a);
int pgo_sparse_graph_add_switchable_edges(pgo_sparse_graph* g, int64_t n, const int32_t* c1, const int32_t* c2, const double* c1_T_c2, const int32_t* switch_idx, const double* ypr_gains,
                                          int32_t loss, double loss_a);
/* pgo_set_node_regularizers' contract: REPLACES the regulariser set */
int pgo_sparse_graph_set_node_regularizers(pgo_sparse_graph* g, int64_t n, const int32_t* node, const double* target, const double* weight);
/* cumulative */
int pgo_sparse_graph_set_nodes_constant(pgo_sparse_graph* g, int64_t n, const int32_t* node);
/* builds the tables (incident lists, free flags, the factor's pair list) and uploads them; allocates the arrays of one linearisation.  No launch. */
int pgo_sparse_graph_finalize(pgo_sparse_graph* g);
/* pgo_evaluate's contract and orders; n_switch: at least every switch index in use + 1.  The gradient of a constant keyframe is zero. */
int pgo_sparse_graph_evaluate(pgo_sparse_graph* g, const double* quat_xyzw, const double* t, const double* sw, int64_t n_nodes, int64_t n_switch, double* cost, double* residuals, double* gradient);
/* pgo_get_normal_blocks' contract and orders, of the last evaluation with a gradient; any pointer may be NULL.  diag and grad of a constant keyframe are zero; grad and sw_gs
 * are the bits pgo_sparse_graph_evaluate returned as the gradient. */
int pgo_sparse_graph_normal_blocks(pgo_sparse_graph* g, double* diag, double* grad, double* offdiag, double* sw_c, double* sw_hss, double* sw_gs);
/* pgo_get_jacobian_blocks' contract, of the last evaluation with a gradient: kind 0 relative-pose, 1 switchable, 2 regulariser */
int pgo_sparse_graph_jacobian_blocks(pgo_sparse_graph* g, int32_t kind, int64_t first, int64_t count, double* J1, double* J2, double* dr_ds);
/* pgo_manifold_plus' contract */
int pgo_sparse_graph_manifold_plus(pgo_sparse_graph* g, int64_t n, const double* quat_xyzw, const double* t, const double* delta, double* quat_out, double* t_out);
/* the three calls above as the callbacks pgo_sparse_lm_solve takes; *user = g */
int pgo_sparse_graph_lm_callbacks(pgo_sparse_graph* g, pgo_sparse_lm_callbacks* cb, void** user);
/* What pgo_sparse_chol_create and pgo_sparse_lm_create need of a finalised graph; any pointer may be NULL (ask counts6 first).  counts6: n_nodes, n_rel, n_sw, n_pairs, the
 * least n_switch, regularisers.  node_free [n_nodes]: 0 for a constant keyframe; in_system [n_nodes]: free and referenced by a block; the edges' endpoints in internal order and
 * every switchable edge's switch index; the pairs of keyframes of the system that an edge joins, each once, pair_hi > pair_lo, sorted.  PGO_ERR_STATE before _finalize. */
int pgo_sparse_graph_edge_lists(const pgo_sparse_graph* g, int64_t* counts6, uint8_t* node_free, uint8_t* in_system, int32_t* rel_c1, int32_t* rel_c2, int32_t* swe_c1, int32_t* swe_c2,
                                int32_t* swe_index, int32_t* pair_hi, int32_t* pair_lo);
/* HIP-event milliseconds of the last pgo_sparse_graph_evaluate: upload of the state, block kernel + cost reduction, node kernel, download.  No launch. */
int pgo_sparse_graph_last_times(const pgo_sparse_graph* g, double* ms4);

/* ---- The reference's 4-DoF pose graph (__USE_YPR_REP, VINS-Fusion's): every keyframe a yaw angle in DEGREES and a translation, every odometry and loop edge a
 * QinFourDOFWeightError (src/CeresResidues.h:426-546) with the pitch and roll of its first keyframe as constants, AngleLocalParameterization on the yaw.  It linearises itself
 * with its own kernels, as pgo_sparse_graph does, and is solved by pgo_sparse_lm_solve as it stands: the graph lives in the six-row slots of the exact LM step.
 *
 * Edge (i, j) with the record (t_meas[3], rel_yaw, pitch_i, roll_i, w), R_i = Rz(psi_i) Ry(pitch_i) Rx(roll_i), N the reference's NormalizeAngle (ONE conditional fold by 360:
 * 180 stays 180, 400 becomes 40, 800 becomes 440):
 *   r[0..2] = w (R_i^T (t_j - t_i) - t_meas)        r[3] = w N(psi_j - psi_i - rel_yaw) / 10
 * Jacobians J1 (keyframe i), J2 (keyframe j): 4 x 4 row-major, columns [psi, t(3)], analytic.  The reference fixes w = 1.  No robust loss, no switch, no regulariser: the
 * reference's 4-DoF path has none.
 *
 * The embedding.  Ambient state: quat[4 i] = psi_i, quat[4 i + 1 .. 4 i + 3] exactly 0 (every call here keeps them 0; a state that has them otherwise is
 * PGO_ERR_INVALID_ARG), t[3 i ..] the translation — so the controller's x_norm, step norm and projected-gradient norm are Ceres' for the parameter blocks (yaw 1, t 3).
 * Tangent: delta[6 i] = dpsi, delta[6 i + 1] = delta[6 i + 2] = 0 (pad), delta[6 i + 3 .. 5] = dt.  Plus: psi+ = N(psi + dpsi), slots 1 - 3 copied, t+ = t + dt.
 * Normal blocks in pgo_get_normal_blocks' layout and orders: diag [n_nodes][36], grad [n_nodes][6], offdiag [n_edges][36] = J1^T J2 per edge in add order.  Pad rows and
 * columns are exactly 0 with ONE exception: on a keyframe of the system (free and referenced by an edge) diag[i][1][1] = diag[i][2][2] = 1.0 exactly — identity rows of the
 * kind the factor keeps for keyframes outside the system.  They keep the undamped matrix positive definite (pgo_sparse_chol_factor and the covariance calls work on it), make
 * dpsi_pad = 0 exactly in every step (zero right-hand side, zero coupling) and add nothing to model_cost_change.  grad pad entries are exactly 0; a constant keyframe gets all
 * zeros.  Cost of the embedding: the factor works on 6 n_nodes rows where a native layout would have 4 n_nodes.
 *
 * One linearisation = pgo_sparse_yaw_graph_evaluate with a gradient: a block kernel (one thread per edge), the one-workgroup cost reduction, a node kernel (one thread per
 * keyframe over its incident list in list order: edge sides in add order).  Cost-only: the block kernel without Jacobians (the same residual bits) and the reduction.  No
 * atomics, one writer per address, nothing waits on another workgroup, every address from the tables of _finalize: two calls give the same bits.  All arrays are host arrays.
 *
 * PGO_ERR_INVALID_ARG — nothing is added, nothing is launched, the text in pgo_sparse_last_error(NULL): a keyframe out of range, an edge from a keyframe to itself, a
 * non-finite number in a record, a weight that is not finite or <= 0.  PGO_ERR_STATE: edges added after _finalize, an evaluation before it, _normal_blocks /
 * _jacobian_blocks before an evaluation with a gradient.  Several edges on one pair, in either direction, a keyframe with no edge, and a graph with no free keyframe in an
 * edge (evaluation works; the solve has an empty system) are all allowed. */
typedef struct pgo_sparse_yaw_graph pgo_sparse_yaw_graph;

int pgo_sparse_yaw_graph_create(int64_t n_nodes, int32_t device_id, pgo_sparse_yaw_graph** out);
void pgo_sparse_yaw_graph_destroy(pgo_sparse_yaw_graph* g);
/* c1: keyframe i (whose pitch and roll the record holds), c2: keyframe j; t_meas [3 n]; rel_yaw, pitch_i, roll_i [n] in degrees; weight [n], NULL: 1 */
int pgo_sparse_yaw_graph_add_edges(pgo_sparse_yaw_graph* g, int64_t n, const int32_t* c1, const int32_t* c2, const double* t_meas, const double* rel_yaw, const double* pitch_i,
                                   const double* roll_i, const double* weight);
/* cumulative */
int pgo_sparse_yaw_graph_set_nodes_constant(pgo_sparse_yaw_graph* g, int64_t n, const int32_t* node);
/* builds the tables (incident lists, free flags, the factor's pair list) and uploads them; allocates the arrays of one linearisation.  No launch. */
int pgo_sparse_yaw_graph_finalize(pgo_sparse_yaw_graph* g);
/* quat [4 n_nodes], t [3 n_nodes]: the ambient state above; residuals [4 n_edges] in add order, gradient [6 n_nodes] in the tangent layout above; cost, residuals, gradient
 * may be NULL */
int pgo_sparse_yaw_graph_evaluate(pgo_sparse_yaw_graph* g, const double* quat, const double* t, int64_t n_nodes, double* cost, double* residuals, double* gradient);
/* of the last evaluation with a gradient; any pointer may be NULL.  grad is the bits pgo_sparse_yaw_graph_evaluate returned as the gradient. */
int pgo_sparse_yaw_graph_normal_blocks(pgo_sparse_yaw_graph* g, double* diag, double* grad, double* offdiag);
/* J1, J2 [count][16] of edges first .. first + count - 1, of the last evaluation with a gradient */
int pgo_sparse_yaw_graph_jacobian_blocks(pgo_sparse_yaw_graph* g, int64_t first, int64_t count, double* J1, double* J2);
/* Plus on n keyframes; t and t_out may be NULL */
int pgo_sparse_yaw_graph_manifold_plus(pgo_sparse_yaw_graph* g, int64_t n, const double* quat, const double* t, const double* delta, double* quat_out, double* t_out);
/* the three calls above as the callbacks pgo_sparse_lm_solve takes (sw = NULL, n_switch = 0; the adapters ignore the sw_* pointers); *user = g */
int pgo_sparse_yaw_graph_lm_callbacks(pgo_sparse_yaw_graph* g, pgo_sparse_lm_callbacks* cb, void** user);
/* What pgo_sparse_chol_create and pgo_sparse_lm_create need of a finalised graph; any pointer may be NULL (ask counts3 first).  counts3: n_nodes, n_edges, n_pairs.
 * node_free [n_nodes]: 0 for a constant keyframe; in_system [n_nodes]: free and referenced by an edge; c1, c2 [n_edges] in add order (pgo_sparse_lm_create's relative-pose
 * edges; it has no switchable ones); the pairs of keyframes of the system that an edge joins, each once, pair_hi > pair_lo, sorted.  PGO_ERR_STATE before _finalize. */
int pgo_sparse_yaw_graph_edge_lists(const pgo_sparse_yaw_graph* g, int64_t* counts3, uint8_t* node_free, uint8_t* in_system, int32_t* c1, int32_t* c2, int32_t* pair_hi, int32_t* pair_lo);
/* HIP-event milliseconds of the last pgo_sparse_yaw_graph_evaluate: upload of the state, block kernel + cost reduction, node kernel, download.  No launch. */
int pgo_sparse_yaw_graph_last_times(const pgo_sparse_yaw_graph* g, double* ms4);

const char* pgo_sparse_strerror(int code);
/* the text of the last error of this object; h = NULL: of the calling thread's last call that had no object (pgo_sparse_spd_solve, pgo_sparse_chol_create, ...) */
const char* pgo_sparse_last_error(const pgo_sparse_chol* h);

#ifdef __cplusplus
}
#endif
#endif
