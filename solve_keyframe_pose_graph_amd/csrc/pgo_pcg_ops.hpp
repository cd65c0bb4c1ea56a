// pgo_pcg_ops.hpp — what the kernels of the PCG iteration share, written once: the reductions, the heads (stop rule, Chronopoulos-Gear scalars, classic alpha), the views of
// CgDev an update works on, the row pair's vector update, the block-Jacobi factors of a trip and the restriction of one keyframe to its aggregate's rigid modes.  Included
// by pgo_kernels.hip inside namespace pgo, ahead of its first kernel; pgo_mg_kernels.hpp (the end of the same translation unit) sees it from there.
// Functions (all __forceinline__: no symbol of their own) where every kernel came out with the instruction stream it had with its own copy, text macros where only those did
// (scripts/dev/kernel_isa_diff.py, profiles/pcg_ops_refactor_check.txt); each macro says what the function form changed.
// The split single-reduction update (cg_update_mg_crit_kernel + the riders of pgo_mg_kernels.hpp) leaves the bits of the unsplit kernel because both expand THESE statements
// (-ffp-contract=on fuses inside one expression only).
// Not here: the prolongation B_i y_a.  Its four users hold it in three shapes — a row pair behind branches (cg_update_restrict_kernel), one component (coarse_pending), all
// six (coarse_prolong_kernel, mf_spmv_kernel's far gather) — and with one text for them coarse_prolong_kernel and mf_spmv_kernel<false, true> came out different.
#pragma once

constexpr int CG_BLOCK = 192;   // 32 keyframes x 6 lanes = 3 wavefronts
constexpr int LF_STRIDE = 24;   // floats per keyframe of the packed block-Jacobi factor (21 used): 6 x 16-B loads

// ------------------------------------------------------------------------------------------------
// reductions (fixed-shape trees: results are bitwise reproducible run to run)
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_down(v, o, 64));
    return v;
}
// This thread's share of a partial-sum array, p[threadIdx.x + k blockDim.x]: up to 12 entries per thread (2 048 partials on 192 lanes) REQUESTED TOGETHER — the loop form
// `for (i = tid; i < n; i += blockDim) v += p[i]` has a run-time trip count, is not unrolled, and waits for every load before it issues the next: four to eleven dependent
// round trips at the head of every PCG kernel, where the whole workgroup waits for alpha / beta (timeline build: 5 us of the matvec's 26).  Same summation order as the loop.
#ifndef PGO_SERIAL_HEAD
__device__ __forceinline__ double strided_share(const double* __restrict__ p, int n) {
    constexpr int MAXK = 12;
    double v[MAXK];
#pragma unroll
    for (int k = 0; k < MAXK; ++k) { const int i = (int)threadIdx.x + k * (int)blockDim.x; v[k] = i < n ? p[i] : 0.0; }
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < MAXK; ++k) s += v[k];
    for (int i = (int)threadIdx.x + MAXK * (int)blockDim.x; i < n; i += blockDim.x) s += p[i];
    return s;
}
#else      // A/B aid (variant build): the loop form
__device__ __forceinline__ double strided_share(const double* __restrict__ p, int n) { double s = 0.0; for (int i = threadIdx.x; i < n; i += blockDim.x) s += p[i]; return s; }
#endif
// sum over the workgroup; valid in thread 0.  `buf` holds blockDim/64 doubles of LDS.
__device__ __forceinline__ double block_sum(double v, double* buf) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    v = wave_sum(v);
    __syncthreads();
    if (lane == 0) buf[wave] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0) for (int i = 0; i < nw; ++i) s += buf[i];
    return s;
}
// Every thread gets the totals of N partial-sum arrays (each a few thousand entries at most, read through L2) in ONE pass: one barrier pair whatever N — every PCG kernel
// starts by re-reducing two of them, the two-level method's three (it keeps the block-Jacobi part and the coarse part of r.z apart).  buf: N x nwaves (+ 1 with FLAG) doubles.
// FLAG, the head of every PCG kernel: "has the PCG stopped?" travels with the re-reduction.  Measured with the timeline build (scripts/dev/mf_timeline.py, C3): as two steps —
// flag -> barrier -> partial sums -> barrier — the head took 5 us of the matvec's 26, two dependent round trips to cold L2s.  Here ONE lane requests the flag BEFORE the
// partial sums are requested and hands it over through the reduction's own LDS buffer: one round trip, one barrier pair.  (The flag may be raised by workgroup 0 of a matvec
// while other workgroups of the same launch are starting: one lane reads, LDS broadcasts, nobody diverges around a barrier.)  Returns the flag (false without FLAG).
template <bool FLAG, int N>
__device__ __forceinline__ bool block_totals(const int32_t* __restrict__ flags, double* buf, const double* __restrict__ pa, int na, double& sa, const double* __restrict__ pb, int nb, double& sb,
                                             const double* __restrict__ pc, int nc, double& sc) {
    static_assert(N >= 1 && N <= 3, "one to three partial-sum arrays");
    int f = 0;
    if (FLAG) { if (threadIdx.x == 0) f = flags[0]; }
    double va = strided_share(pa, na), vb = 0.0, vc = 0.0;
    if (N > 1) vb = strided_share(pb, nb);
    if (N > 2) vc = strided_share(pc, nc);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    va = wave_sum(va);
    if (N > 1) vb = wave_sum(vb);
    if (N > 2) vc = wave_sum(vc);
    __syncthreads();
    if (lane == 0) { buf[wave] = va; if (N > 1) buf[nw + wave] = vb; if (N > 2) buf[2 * nw + wave] = vc; }
    if (FLAG) { if (threadIdx.x == 0) buf[N * nw] = (double)f; }
    __syncthreads();
    sa = 0.0; if (N > 1) sb = 0.0; if (N > 2) sc = 0.0;
    for (int i = 0; i < nw; ++i) { sa += buf[i]; if (N > 1) sb += buf[nw + i]; if (N > 2) sc += buf[2 * nw + i]; }
    return FLAG && buf[N * nw] != 0.0;
}
// (two arrays, one array: the arguments a smaller N never touches are filled in)
template <bool FLAG>
__device__ __forceinline__ bool block_totals(const int32_t* __restrict__ flags, double* buf, const double* __restrict__ pa, int na, double& sa, const double* __restrict__ pb, int nb, double& sb) {
    return block_totals<FLAG, 2>(flags, buf, pa, na, sa, pb, nb, sb, nullptr, 0, sb);
}
__device__ __forceinline__ double block_total(const double* __restrict__ partials, int n, double* buf) { double s; block_totals<false, 1>(nullptr, buf, partials, n, s, nullptr, 0, s, nullptr, 0, s); return s; }

// ------------------------------------------------------------------------------------------------
// heads: what every workgroup of a PCG kernel decides, from the same numbers, before it touches a vector
// ------------------------------------------------------------------------------------------------
// The stop rule on the preconditioned residual norm rz = r.z (every workgroup evaluates the same numbers -> uniform exit).  True: converged or broken down — flags[0] is
// raised, the state stays that of the last completed update, scal[1] keeps r.z; a clearly negative r.z means the preconditioner is not positive definite: a breakdown, never
// convergence.  coarse_negative (two-level method; false where there is no coarse part): the coarse term alone pulled r.z below the tolerance (sr_head, mf_spmv_kernel).
__device__ __forceinline__ bool pcg_stopped(const CgDev& C, double rz, bool coarse_negative) {
    const bool breakdown = C.flags[1] != 0;
    if (breakdown || !(rz > C.scal[3] * C.scal[0])) {
        if (blockIdx.x == 0 && threadIdx.x == 0) { C.flags[0] = 1; if (!breakdown) { C.scal[1] = rz; if (coarse_negative || !(rz >= -C.scal[3] * C.scal[0])) C.flags[1] = 1; } }
        return true;
    }
    return false;
}
// beta of the single-reduction (Chronopoulos-Gear) form from the gamma the head of the previous iteration left in scal[8 + 2 (parity ^ 1)]
__device__ __forceinline__ double sr_beta(const double* __restrict__ scal, int parity, int first, double gamma) {
    if (first) return 0.0;
    const double gamma_prev = scal[8 + 2 * (parity ^ 1)];
    return gamma / gamma_prev;
}
// The Chronopoulos-Gear scalars from delta = u.w and gamma = r.u: the stop rule the classic form runs at the head of its matvec, beta = gamma / gamma_prev,
// alpha = gamma / (delta - beta gamma / alpha_prev).  Scalars in C.scal[8 + 2 parity] (gamma), [9 + 2 parity] (alpha) of the iteration with that parity.  False: the
// workgroup has nothing to do (converged, broken down).
__device__ __forceinline__ bool sr_scalars(const CgDev& C, int parity, int first, double delta, double gamma, bool coarse_negative, double& alpha, double& beta) {
    if (pcg_stopped(C, gamma, coarse_negative)) return false;
    beta = sr_beta(C.scal, parity, first, gamma);
    double den = delta;
    if (!first) { const double alpha_prev = C.scal[9 + 2 * (parity ^ 1)]; den = delta - beta * gamma / alpha_prev; }
    if (!(den > 0.0)) {      // not positive definite along the direction (or NaN): x is left untouched
        if (blockIdx.x == 0 && threadIdx.x == 0) { C.flags[1] = 1; C.flags[0] = 1; }
        return false;
    }
    alpha = gamma / den;
    if (blockIdx.x == 0 && threadIdx.x == 0) { C.scal[8 + 2 * parity] = gamma; C.scal[9 + 2 * parity] = alpha; C.scal[1] = gamma; C.flags[2] += 1; }
    return true;
}
// The head of the single-reduction update on one GPU: delta = u.w (the matvec's partials) and gamma = r.u (the previous update's) are re-reduced TOGETHER — the iteration's
// only reduction point — then sr_scalars.  Returns false when the workgroup has nothing to do (stopped, converged, broken down).
// split_coarse (the two-level method's fused iteration): the slots behind the update kernel's `nparts` hold the coarse part rc.Ac^-1 rc of r.u (coarse_solve_dot_kernel); a
// convergence that the block-Jacobi part alone does not confirm is a breakdown of the fp32-rounded coarse inverse, never a converged step (the classic form runs the same
// test at the head of its matvec: mf_spmv_kernel<true, true>); coarse_only: one aggregate per keyframe, u is the coarse term alone.  red: 3 x waves + 1 doubles then.
__device__ __forceinline__ bool sr_head(const CgDev& C, int parity, int first, int nparts_pq, int nparts, double* red, double& alpha, double& beta, bool split_coarse = false, bool coarse_only = false) {
    double delta, gamma;
    bool coarse_negative = false;
    if (split_coarse) {
        double g_bj, g_c;
        if (block_totals<true, 3>(C.flags, red, C.part_pq, nparts_pq, delta, C.part_rz + parity * RZ_STRIDE, nparts, g_bj, C.part_rz + parity * RZ_STRIDE + nparts, C.extra_rz, g_c)) return false;
        gamma = g_bj + g_c;
        coarse_negative = !coarse_only && !(gamma > C.scal[3] * C.scal[0]) && g_bj > C.scal[3] * C.scal[0];
    } else if (block_totals<true>(C.flags, red, C.part_pq, nparts_pq, delta, C.part_rz + parity * RZ_STRIDE, nparts + C.extra_rz, gamma)) return false;
    return sr_scalars(C, parity, first, delta, gamma, coarse_negative, alpha, beta);
}
// The head of an update kernel, single-reduction (sr_head) or classic: p.q (the matvec's partials, its own grid size) and r.z re-reduced with the flag, alpha = rz / pq.
// It RETURNS from the kernel when the workgroup has nothing to do: stopped, or a breakdown — the matrix is not positive definite along p (or NaN): x is left untouched, the
// workgroup's r.z partial is zeroed and the next matvec raises done.  A macro: as a function that reports "nothing to do" the classic head's two exits were laid out
// differently in all three update kernels (profiles/pcg_ops_refactor_check.txt).
#define PCG_UPDATE_HEAD_OR_RETURN(SR, C, parity, first, nparts_pq, nparts, red, alpha, beta, ...)                                                  \
    if (SR) { if (!sr_head(C, parity, first, nparts_pq, nparts, red, alpha, beta, ##__VA_ARGS__)) return; }                                        \
    else {                                                                                                                                         \
        double pq, rz;                                                                                                                             \
        if (block_totals<true>(C.flags, red, C.part_pq, nparts_pq, pq, C.part_rz + parity * RZ_STRIDE, nparts + C.extra_rz, rz)) return;           \
        if (!(pq > 0.0)) {                                                                                                                         \
            if (blockIdx.x == 0 && threadIdx.x == 0) C.flags[1] = 1;                                                                               \
            if (threadIdx.x == 0) C.part_rz[(parity ^ 1) * RZ_STRIDE + blockIdx.x] = 0.0;                                                          \
            return;                                                                                                                                \
        }                                                                                                                                          \
        alpha = rz / pq;                                                                                                                           \
    }

// ------------------------------------------------------------------------------------------------
// the vector update of one row pair: one lane per (keyframe, ROW PAIR), every vector access 16 B/lane (8-B accesses reach only ~0.6x of the streaming rate)
// ------------------------------------------------------------------------------------------------
// classic form (SR = false):   x += alpha p ; r' = r - alpha q        (r/r2 and p/p2 ping-pong by iteration parity)
// single-reduction form (SR):  p = u + beta p ; s = w + beta s ; x += alpha p ; r -= alpha s        (u in C.z, w in C.q, s in C.p2, r and p in place)
template <bool SR>
struct UpdateViews {
    const double2* __restrict__ rin; double2* __restrict__ rout; const double2* __restrict__ pcur; const double2* __restrict__ qv;
    double2* __restrict__ xv; double2* __restrict__ zv;
    double2* __restrict__ pout;      // (SR only)
    double2* __restrict__ sv;        // (SR only) s = A p
    __device__ __forceinline__ UpdateViews(const CgDev& C, int parity)
        : rin(reinterpret_cast<const double2*>(SR ? C.r : (parity ? C.r2 : C.r))), rout(reinterpret_cast<double2*>(SR ? C.r : (parity ? C.r : C.r2))),
          pcur(reinterpret_cast<const double2*>(SR ? C.p : (parity ? C.p2 : C.p))), qv(reinterpret_cast<const double2*>(C.q)), xv(reinterpret_cast<double2*>(C.x)),
          zv(reinterpret_cast<double2*>(C.z)), pout(reinterpret_cast<double2*>(C.p)), sv(reinterpret_cast<double2*>(C.p2)) {}
};
// The three statements on a row pair (double2).  Macros, as is PCG_UPDATE_PAIR: with functions taking the operands by reference cg_update_restrict_kernel allocated their
// registers in another order (profiles/pcg_ops_refactor_check.txt).
#define PAIR_XPBY(beta, U, P) { P.x = U.x + beta * P.x; P.y = U.y + beta * P.y; }                      /* P = U + beta P */
#define PAIR_AXPY(alpha, P, X) { X.x += alpha * P.x; X.y += alpha * P.y; }                             /* X += alpha P */
#define PAIR_MINUS(RR, alpha, R, S) { RR = make_double2(R.x - alpha * S.x, R.y - alpha * S.y); }       /* RR = R - alpha S */
// Row pair i of the views V: the operands in registers (r0 q0 p0 x0, SR: u0 s0) become the new p, s, x in place and are stored; the new residual goes to rr and is stored.
// CRIT (single-reduction form only): the half the multigrid cycle waits for — s and r; p and x are upd_rider_direction's (pgo_mg_kernels.hpp).
#define PCG_UPDATE_PAIR(SR, CRIT, V, i, alpha, beta, r0, q0, p0, x0, u0, s0, rr)     \
    {                                                                                \
        if (SR) {                                                                    \
            if (!CRIT) PAIR_XPBY(beta, u0, p0)                                       \
            PAIR_XPBY(beta, q0, s0)                                                  \
            PAIR_MINUS(rr, alpha, r0, s0)                                            \
            if (!CRIT) { PAIR_AXPY(alpha, p0, x0) V.pout[i] = p0; }                  \
            V.sv[i] = s0;                                                            \
        } else {                                                                     \
            PAIR_MINUS(rr, alpha, r0, q0)                                            \
            PAIR_AXPY(alpha, p0, x0)                                                 \
        }                                                                            \
        V.rout[i] = rr;                                                              \
        if (!CRIT) V.xv[i] = x0;                                                     \
    }

// ------------------------------------------------------------------------------------------------
// the block-Jacobi factors of a workgroup trip (CG_BLOCK / 3 keyframes from `first_node`): two 16-B loads per lane, staged through registers — they travel with the trip's
// vector operands, not behind a barrier of their own — then into LDS beside the trip's new residual
// ------------------------------------------------------------------------------------------------
// Macros both: `t` is the caller's thread index as it holds it (threadIdx.x or an int copy — the index arithmetic keeps its signedness), and as functions the kernels
// computed the LDS addresses and allocated registers in another order; for the same reason the callers of LF_TRIP_APPLY form the two LDS addresses themselves.
static_assert((CG_BLOCK / 3) * LF_STRIDE / 4 == 2 * CG_BLOCK, "two 16-B loads per lane stage a trip's factors");
#define LF_TRIP_LOAD(Lf, first_node, N, t, l0, l1)                                                                       \
    {                                                                                                                    \
        const float4* lp = reinterpret_cast<const float4*>(Lf + (size_t)(first_node) * LF_STRIDE);                       \
        if ((first_node) + (t) / 6 < N) l0 = lp[t];                                                                      \
        if ((first_node) + ((t) + CG_BLOCK) / 6 < N) l1 = lp[(t) + CG_BLOCK];                                            \
    }
// z = (L L^T)^-1 r of the lane's row pair j from its keyframe's factors Lf and six residual entries r6, both in LDS -> zout; rz = the lane's term r.z
#define LF_TRIP_APPLY(Lf, r6, j, rr, zout, rz)           \
    const double2 z = lf_apply_pair(Lf, r6, j);          \
    zout = z;                                            \
    const double rz = rr.x * z.x + rr.y * z.y;

// ------------------------------------------------------------------------------------------------
// the rigid-mode restriction of one keyframe i at offset d_i from its aggregate's centroid, by row pair j (rows 2j, 2j + 1)
// ------------------------------------------------------------------------------------------------
// b = B_i^T r_i = [r_theta + 2 d_i x r_t ; r_t], r6 the keyframe's six residual entries.  A macro: as a function cg_update_restrict_kernel<false> came out with
// other registers throughout (profiles/pcg_ops_refactor_check.txt).
#define RIGID_RESTRICT_PAIR(b, r6, j, d0, d1, d2)                                                                                         \
    {                                                                                                                                     \
        if (j == 0) b = make_double2(r6[0] + 2.0 * (d1 * r6[5] - d2 * r6[4]), r6[1] + 2.0 * (d2 * r6[3] - d0 * r6[5]));                   \
        else if (j == 1) b = make_double2(r6[2] + 2.0 * (d0 * r6[4] - d1 * r6[3]), r6[3]);                                                \
        else b = make_double2(r6[4], r6[5]);                                                                                              \
    }
