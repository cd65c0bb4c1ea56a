// pgo_measure.hip — measurement helpers and test diagnostics of the C-ABI: HIP-event times and algorithmic bytes of the solver's kernels on the state of an open solve
// (pgo_time_kernel), of K0 (pgo_time_vio_odometry_kernel), of the dense inverse (pgo_dense_spd_inverse), of the dense Cholesky solve (pgo_dense_spd_solve) and of its covariance blocks (pgo_dense_spd_covariance), the sums of squares of a multigrid level's operators
// (pgo_mg_level_norms), a preconditioner applied to the caller's vectors (pgo_apply_preconditioner), the last PCG's iterate (pgo_get_linear_solution), the installed
// hierarchy's aggregates (pgo_mg_level_parents), the matrix-free operator's tile tables (pgo_get_matrix_free_tiles) and the normal operator applied to a batch of vectors
// (pgo_apply_normal_operator_batch).  Nothing here runs inside a solve's own steps.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "pgo_handle.hpp"
#include "pgo_dense_math.hpp"

namespace {

// ---- pgo_time_kernel: what it measures
//   0  K1 with Jacobians at the current state        3  K1 without Jacobians at the candidate state        1  K2
//   2  one PCG iteration of the form the solver runs on this handle, block-Jacobi preconditioner (several ranks: the rank's own iteration, no exchanges);
//   4  its matvec alone;  5  its vector update alone
//   6  one multigrid-preconditioned PCG iteration;  7  the cycle's level kernels alone (several ranks: this rank's share, no exchanges)
//   8  this rank's kernels of one multigrid set-up (operators of an LM system incl. the dense inverse), without the exchanges between them

// What a diagnostic that builds an LM system of its own at `radius` (<= 0: the current one) leaves as it found it: the radius, and the two-level method's comparison state
// (build_lm_system may spend a retest).  No preconditioner stays active behind it.
struct ProbeRestore {
    pgo_problem* p; double radius; int mode, retests;
    ProbeRestore(pgo_problem* q, double r) : p(q), radius(q->lm.radius), mode(q->coarse.hist.mode), retests(q->coarse.hist.retests) { if (r > 0.0) p->lm.radius = r; }
    ~ProbeRestore() { p->lm.radius = radius; p->coarse.hist.mode = mode; p->coarse.hist.retests = retests; p->mg.active = false; p->coarse.active = false; p->C.extra_rz = 0; }
};

// 2 / 4 / 5: a live block-Jacobi PCG state to iterate on (tolerance 0: never converges during the timed launches)
int setup_block_jacobi(pgo_problem* p) {
    int rc; bool ok = true;
    if ((rc = build_lm_system(p, &ok)) != PGO_OK) return rc;
    p->mg.active = false; p->coarse.active = false; p->C.extra_rz = 0;   // the timed iteration is the plain block-Jacobi one: no partial-sum slots of a multigrid / two-level solve
    launch_cg_init(p->G, p->C, 0, 0.0, p->st);
    return PGO_OK;
}

// 6 / 7 / 8: the multigrid operators of the current LM system and a live PCG state on them
int setup_multigrid(pgo_problem* p, int which) {
    if (!p->mg.built || !p->built_mf || (p->local_ids && which == 6)) { p->err = "pgo_time_kernel: this graph has no multigrid hierarchy (mg_min_keyframes) / several ranks: only the level kernels (7) can be timed"; return PGO_ERR_STATE; }
    int rc; bool ok = true;
    if ((rc = build_lm_system(p, &ok)) != PGO_OK) return rc;
    if (!p->mg.active && (rc = build_mg(p)) != PGO_OK) return rc;
    if (!p->mg.active) { p->err = "pgo_time_kernel: the multigrid operators of this system are not positive definite"; return PGO_ERR_NUMERIC; }
    if (!p->local_ids) return pcg_start(p, choose_form(p), false, 0.0);      // (tolerance 0: never converges during the timed launches)
    launch_cg_init_vectors(p->G, p->C, 0, p->st);
    if ((rc = mg_apply_ranks(p, false)) != PGO_OK) return rc;      // (one full distributed cycle: every level vector holds finite numbers)
    launch_cg_set_tolerance(p->C, 0.0, p->st);
    return PGO_OK;
}

// the form measurement `which` (6 / 7) runs: 7 is the cycle alone — the restriction is its own, no update in front and no riders
PcgForm multigrid_form(const pgo_problem* p, int which) {
    PcgForm f = choose_form(p);
    if (which == 7) { f.post = PcgForm::mg_cycle; f.split = UpdSplit{}; }
    return f;
}

// one launch of measurement `which`; kk: the PCG iteration it stands for (0: the untimed launch)
int enqueue(pgo_problem* p, int which, int kk) {
    const GraphDev& G = p->G;
    int np = 0, rc;
    switch (which) {
        case 0: launch_k1(G, p->d_pose[p->cur].p, p->d_swv[p->cur].p, true, part(p, 0), &np, p->st); return PGO_OK;
        case 1: launch_k2(G, p->L, !p->built_mf, p->st, p->built_mf ? &p->F : nullptr); return PGO_OK;
        case 2: case 4: case 5: {
            const PcgForm f = choose_form(p, true);      // the form the solver runs on this handle (several ranks: the rank's own iteration, no exchanges)
            if (which != 5) pcg_matvec(p, f, kk, 0.0);
            return which != 4 ? pcg_update(p, f, kk) : PGO_OK; }
        case 3: launch_k1(G, p->d_pose[p->cur ^ 1].p, p->d_swv[p->cur ^ 1].p, false, part(p, 5), &np, p->st); return PGO_OK;
        case 6: case 7: {
            if (p->local_ids) {      // several ranks (7 only): this rank's share of the cycle's kernels, no exchanges (what its GPU computes per cycle)
                mg_cycle(p, p->C, MgCycleArgs{});
                return PGO_OK;
            }
            const PcgForm f = multigrid_form(p, which);
            if (which == 6) { pcg_matvec(p, f, kk, 0.0); if ((rc = pcg_update(p, f, kk)) != PGO_OK) return rc; }
            return pcg_precond(p, f, kk); }
        case 8: return mg_operators(p, p->coarse.d_cinfo.p, !p->built_mf || p->hoff_epoch == p->lin_epoch, true, -1.0);
        default: return PGO_ERR_INVALID_ARG;
    }
}

// Bytes the fine-level PCG iteration moves, each array once.  Matrix-free matvec: per LANE (a relative-pose edge with both keyframes in one tile is one lane, every other edge
// side its own) the compact record (8 double2 planes; 11 for switchable sides) + 12 B of index data (+ a_inv for switchable sides); per keyframe z and p_prev read, p and q
// written (4 x 48), damping 48, side ranges / regulariser index / free flag 13.  Update: r, q, p, x read, r, x, z written (7 x 48), the fp32 block-Jacobi factor 96.
// Block-CSR matvec: SURVEY.md 8d's assembled form.  Single-reduction form (sr): the matvec reads u and writes w (2 x 48 per keyframe instead of 4 x 48); the update reads
// u, w, p, s, x, r and writes p, s, x, r, u (11 x 48).
struct FineBytes { double matvec, update; };
FineBytes fine_iteration_bytes(const pgo_problem* p, bool sr) {
    const double N = (double)p->G.N, E = (double)(p->G.rel.E + p->G.sw.E);
    const double lanes_rel = (double)(p->mf_pair_lanes + p->mf_rel_side_lanes), lanes_sw = (double)p->mf_sw_lanes;
    const double mv = p->built_mf ? lanes_rel * (128.0 + 12.0) + lanes_sw * (128.0 + 12.0 + 8.0) + N * ((sr ? 2.0 : 4.0) * 48.0 + 48.0 + 13.0)
                                  : 288.0 * (N + 2.0 * E) + 4.0 * (N + 2.0 * E) + N * 4.0 * 48.0;
    return FineBytes{mv, N * ((sr ? 11.0 : 7.0) * 48.0 + 96.0)};
}

// Bytes of the multigrid cycle, each array once per kernel that streams it: the restriction's per-keyframe offsets and slot table, the prolongation's read-modify-write of z,
// offsets and aggregate index; every sparse coarse level: its fp32 blocks and column indices twice (down- and up-sweep), Dinv, positions/offsets and its four vectors; the
// dense level: the fp32 inverse once.
double cycle_bytes(const pgo_problem* p, bool split_update) {
    const double N = (double)p->G.N;
    double cyc = N * (24.0 + 16.0 / 8.0 * 8.0) /* d0 + slot table (restriction) */ + N * (2.0 * 48.0 + 24.0 + 4.0 + 4.0) /* z read + write, d0, agg0, member list (prolongation) */;
    for (int l = 0; l + 1 < p->mg.M.n_levels; ++l) {
        const MgLevelDev& A = p->mg.levels[l];
        if (mg_explicit(A))      // explicit transfer operator: the level's own blocks once (smoothing step), R and R^T once each, Dinv once, r / x / y / xf and the level above's r, x
            cyc += (double)A.nnzb * (144.0 + 4.0) + 2.0 * (double)A.n_w * (144.0 + 4.0) + (double)A.n * (288.0 + 24.0 + 8.0 * 48.0 + 16.0) + (double)A.n_next * (288.0 + 2.0 * 48.0 + 8.0);
        else
            cyc += (A.smoothed ? 4.0 : 2.0) * (double)A.nnzb * (144.0 + 4.0) + (double)A.n * ((A.smoothed ? 4.0 : 2.0) * 288.0 /* Dinv: smoothing steps */ + 24.0 + (A.smoothed ? 18.0 : 10.0) * 48.0 + 16.0);
    }
    cyc += (double)p->coarse.K.nc * (double)p->coarse.K.nc * 4.0 + (double)p->coarse.K.nc * 16.0;
    if (split_update) cyc += N * 48.0;      // the split update: the block-Jacobi rider reads the new residual back
    return cyc;
}

// what one launch of measurement `which` moves, on the state its set-up left
double algorithmic_bytes(const pgo_problem* p, int which) {
    const GraphDev& G = p->G;
    const double N = (double)G.N, E = (double)(G.rel.E + G.sw.E), Es = (double)G.sw.E;
    switch (which) {
        case 0: return k1_algorithmic_bytes(G, true);
        case 1: return (624.0 * G.rel.E + 688.0 * Es) + 288.0 * E + 336.0 * N + 112.0 * Es;
        case 2: case 4: case 5: {
            const FineBytes fine = fine_iteration_bytes(p, choose_form(p, true).single_red());
            return which == 2 ? fine.matvec + fine.update : which == 4 ? fine.matvec : fine.update; }
        case 3: return k1_algorithmic_bytes(G, false);
        case 6: case 7: {
            if (p->local_ids) return (double)p->mg.blocks_own * 148.0 + (double)p->mg.rows_own * (288.0 + 24.0 + 8.0 * 48.0 + 16.0) + (double)p->coarse.K.nc * (double)p->coarse.K.nc * 4.0 + (double)p->coarse.K.nc * 16.0;
            const PcgForm f = multigrid_form(p, which);
            const double cyc = cycle_bytes(p, f.split.on());
            if (which == 7) return cyc;
            const FineBytes fine = fine_iteration_bytes(p, f.single_red());
            return fine.matvec + fine.update + cyc; }
        default: return 0.0;
    }
}

// One untimed launch first (instruction cache, TLB), then `batches` x `launches` between events; the fastest batch counts.  Several ranks (7 / 8): the timed launches take
// turns (every rank's figure is what its GPU would need on its own); only the in-process ranks, which share the GPU(s), wait for each other.  In-process ranks: three timed
// batches — the first batch after a solve_begin that regrouped the hierarchy was measured at 3-5x the steady figure on every rank (C5 on 8 ranks: 0.47-0.82 ms, then
// 0.146-0.168 ms call after call): eight handles' old images going back to the system stall the GPU's address translation for tens of milliseconds.
int time_launches(pgo_problem* p, int which, int launches, double* best_ms) {
    int rc;
    EventPair ev;
    HIPCHK(p, ev.create());
    const int turns = (p->comm && (which == 7 || which == 8)) ? p->world() : 1;
    const int batches = turns > 1 ? 3 : 1;
    *best_ms = -1.0;
    for (int turn = 0; turn < turns; ++turn) {
        if (turns > 1) {
            HIPCHK(p, hipStreamSynchronize(p->st));
            if (!p->comm->barrier()) { p->err = "in-process communicator: a rank left during pgo_time_kernel"; return PGO_ERR_COMM; }
            if (turn != p->rank()) continue;
        }
        for (int rep = 0; rep < 1 + batches; ++rep) {
            const int n = rep == 0 ? 1 : launches;
            if (rep >= 1) HIPCHK(p, hipEventRecord(ev.e0, p->st));
            for (int i = 0; i < n; ++i) if ((rc = enqueue(p, which, rep == 0 ? 0 : i + 1)) != PGO_OK) return rc;
            if (rep >= 1) HIPCHK(p, hipEventRecord(ev.e1, p->st));
            HIPCHK(p, hipStreamSynchronize(p->st));
            if (rep >= 1) { float msb = 0; HIPCHK(p, hipEventElapsedTime(&msb, ev.e0, ev.e1)); if (*best_ms < 0.0 || (double)msb < *best_ms) *best_ms = (double)msb; }
        }
    }
    if (turns > 1 && !p->comm->barrier()) { p->err = "in-process communicator: a rank left during pgo_time_kernel"; return PGO_ERR_COMM; }
    return PGO_OK;
}

}  // namespace

extern "C" {

int pgo_time_kernel(pgo_problem* p, int32_t which, int32_t launches, double* avg_ms, double* algorithmic_bytes_out) {
    if (!p || launches <= 0 || !avg_ms) return PGO_ERR_INVALID_ARG;
    if (!p->in_solve) { p->err = "pgo_time_kernel needs an open solve (pgo_solve_begin)"; return PGO_ERR_STATE; }
    int rc;
    if ((rc = set_device(p)) != PGO_OK) return rc;
    if (which < 0 || which > 8) return PGO_ERR_INVALID_ARG;
    if (which == 5 && single_reduction(p)) {      // (its head needs the u.w partials of a matvec on the CURRENT u: launched back to back it sees stale ones, breaks down and returns early)
        p->err = "pgo_time_kernel(5): the single-reduction update cannot be timed without its matvec; time the iteration (2) and the matvec (4) and subtract"; return PGO_ERR_STATE;
    }
    if ((which == 2 || which == 4 || which == 5) && (rc = setup_block_jacobi(p)) != PGO_OK) return rc;
    if (which >= 6 && (rc = setup_multigrid(p, which)) != PGO_OK) return rc;
    const double bytes = algorithmic_bytes(p, which);
    double best_ms = -1.0;
    if ((rc = time_launches(p, which, launches, &best_ms)) != PGO_OK) return rc;
    if (which == 8) { p->mg.active = false; if ((rc = build_mg(p)) != PGO_OK) return rc; }      // (several ranks: the timed kernels ran without their exchanges — the operators are formed again, properly)
    *avg_ms = best_ms / launches;
    if (algorithmic_bytes_out) *algorithmic_bytes_out = bytes;
    return PGO_OK;
}
int pgo_time_linearize_kernel(pgo_problem* p, int32_t launches, double* avg_ms, double* bytes) { return pgo_time_kernel(p, 0, launches, avg_ms, bytes); }

int pgo_time_vio_odometry_kernel(pgo_problem* p, int32_t f_max, int32_t launches, double* avg_ms, double* algorithmic_bytes) {
    if (!p || launches <= 0 || !avg_ms || f_max < 1) return PGO_ERR_INVALID_ARG;
    if (p->n_vio < 2) { p->err = "no resident VIO poses"; return PGO_ERR_STATE; }
    int rc;
    if ((rc = set_device(p)) != PGO_OK) return rc;
    std::vector<int32_t> c;
    for (int64_t u = 0; u < p->n_vio; ++u) for (int f = 1; f <= f_max; ++f) if (u - f >= 0) c.push_back((int32_t)u);
    const int64_t n = (int64_t)c.size();
    for (int64_t u = 0; u < p->n_vio; ++u) for (int f = 1; f <= f_max; ++f) if (u - f >= 0) c.push_back((int32_t)(u - f));
    DBuf<int32_t> d_c; DBuf<double> d_meas;
    HIPCHK(p, d_c.ensure((size_t)2 * n)); HIPCHK(p, d_meas.ensure((size_t)8 * n));
    HIPCHK(p, hipMemcpyAsync(d_c.p, c.data(), (size_t)2 * n * sizeof(int32_t), hipMemcpyHostToDevice, p->st));
    EventPair ev;
    HIPCHK(p, ev.create());
    const hipEvent_t e0 = ev.e0, e1 = ev.e1;
    launch_vio_odometry(n, d_c.p, d_c.p + n, p->d_vio.p, 1, d_meas.p, p->st);
    HIPCHK(p, hipEventRecord(e0, p->st));
    for (int i = 0; i < launches; ++i) launch_vio_odometry(n, d_c.p, d_c.p + n, p->d_vio.p, 1, d_meas.p, p->st);
    HIPCHK(p, hipEventRecord(e1, p->st));
    HIPCHK(p, hipStreamSynchronize(p->st));
    float ms = 0;
    HIPCHK(p, hipEventElapsedTime(&ms, e0, e1));
    *avg_ms = (double)ms / launches;
    if (algorithmic_bytes) *algorithmic_bytes = 128.0 * (double)p->n_vio + (8.0 + 64.0) * (double)n;   // each pose once + 2 indices + one record per edge
    return PGO_OK;
}

int pgo_dense_spd_inverse(pgo_problem* p, int32_t n, const double* a, double* a_inv, int32_t launches, double* avg_ms) {
    if (!p || n <= 0 || !a || !a_inv || launches < 1) return PGO_ERR_INVALID_ARG;
    int rc;
    if ((rc = set_device(p)) != PGO_OK) return rc;
    const int nc = (n + 63) / 64 * 64;
    std::vector<double> h((size_t)nc * nc, 0.0);
    for (int i = 0; i < nc; ++i) {
        if (i < n) std::memcpy(&h[(size_t)i * nc], a + (size_t)i * n, (size_t)n * sizeof(double));
        else h[(size_t)i * nc + i] = 1.0;
    }
    DBuf<double> d_a, d_scr; DBuf<int32_t> d_fail;
    HIPCHK(p, d_a.ensure((size_t)nc * nc)); HIPCHK(p, d_scr.ensure((size_t)nc * 64 + 4096)); HIPCHK(p, d_fail.ensure(1));
    CoarseDev K{}; K.nc = nc; K.Ac = d_a.p;
    EventPair ev;
    HIPCHK(p, ev.create());
    const hipEvent_t e0 = ev.e0, e1 = ev.e1;
    float total = 0;
    for (int l = 0; l < launches; ++l) {
        HIPCHK(p, hipMemcpyAsync(d_a.p, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, p->st));
        HIPCHK(p, hipMemsetAsync(d_fail.p, 0, sizeof(int32_t), p->st));
        HIPCHK(p, hipEventRecord(e0, p->st));
        launch_coarse_invert(K, d_scr.p, d_fail.p, p->st);
        HIPCHK(p, hipEventRecord(e1, p->st));
        HIPCHK(p, hipStreamSynchronize(p->st));
        float ms = 0;
        HIPCHK(p, hipEventElapsedTime(&ms, e0, e1));
        total += ms;
    }
    int32_t fail = 1;
    HIPCHK(p, hipMemcpy(&fail, d_fail.p, sizeof(fail), hipMemcpyDeviceToHost));
    HIPCHK(p, hipMemcpy(h.data(), d_a.p, h.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) std::memcpy(a_inv + (size_t)i * n, &h[(size_t)i * nc], (size_t)n * sizeof(double));
    if (avg_ms) *avg_ms = (double)total / launches;
    if (fail) { p->err = "matrix is not numerically positive definite"; return PGO_ERR_NUMERIC; }
    return PGO_OK;
}

int pgo_dense_spd_solve(pgo_problem* p, int32_t n, const double* a, const double* b, double* x, int32_t launches, double* avg_ms) {
    if (!p || n <= 0 || !a || !b || !x || launches < 1) return PGO_ERR_INVALID_ARG;
    int rc;
    if ((rc = set_device(p)) != PGO_OK) return rc;
    const int nc = (n + 63) / 64 * 64;
    std::vector<double> h((size_t)nc * nc, 0.0), hb((size_t)nc, 0.0);
    for (int i = 0; i < nc; ++i) {
        if (i < n) { std::memcpy(&h[(size_t)i * nc], a + (size_t)i * n, (size_t)n * sizeof(double)); hb[i] = b[i]; }
        else h[(size_t)i * nc + i] = 1.0;
    }
    DBuf<double> d_a, d_scr, d_vec, d_x; DBuf<int32_t> d_fail;
    HIPCHK(p, d_a.ensure((size_t)nc * nc)); HIPCHK(p, d_scr.ensure(dense_scratch_doubles(nc))); HIPCHK(p, d_vec.ensure((size_t)2 * nc)); HIPCHK(p, d_x.ensure((size_t)nc)); HIPCHK(p, d_fail.ensure(1));
    EventPair ev;
    HIPCHK(p, ev.create());
    float total = 0;
    int32_t fail = 0;
    for (int l = 0; l < launches && !fail; ++l) {
        HIPCHK(p, hipMemcpyAsync(d_a.p, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, p->st));
        HIPCHK(p, hipMemcpyAsync(d_vec.p, hb.data(), hb.size() * sizeof(double), hipMemcpyHostToDevice, p->st));
        HIPCHK(p, hipMemsetAsync(d_fail.p, 0, sizeof(int32_t), p->st));
        HIPCHK(p, hipEventRecord(ev.e0, p->st));
        launch_dense_factor(d_a.p, nc, d_scr.p, d_fail.p, false, p->st);
        launch_dense_solve(d_a.p, nc, d_vec.p, d_vec.p + nc, d_x.p, nc, p->st);      // (a failed factor: the sweeps run on numbers nobody reads — inside their own buffers)
        HIPCHK(p, hipEventRecord(ev.e1, p->st));
        HIPCHK(p, hipMemcpyAsync(&fail, d_fail.p, sizeof(fail), hipMemcpyDeviceToHost, p->st));
        HIPCHK(p, hipStreamSynchronize(p->st));
        float ms = 0;
        HIPCHK(p, hipEventElapsedTime(&ms, ev.e0, ev.e1));
        total += ms;
    }
    if (avg_ms) *avg_ms = (double)total / launches;
    if (fail) { p->err = "matrix is not numerically positive definite"; return PGO_ERR_NUMERIC; }
    HIPCHK(p, hipMemcpy(hb.data(), d_x.p, hb.size() * sizeof(double), hipMemcpyDeviceToHost));
    std::memcpy(x, hb.data(), (size_t)n * sizeof(double));
    return PGO_OK;
}

// The covariance launches on a symmetric positive definite matrix and n_sw >= 0 switch columns, arguments checked by the two hooks below: the right-hand sides, the
// factorisation, the substitutions and the Gram products between one pair of events, `launches` times
static int dense_spd_covariance_launches(pgo_problem* p, int32_t n, const double* a, int32_t n_sw, const int32_t* sw_node, const double* sw_c, const double* sw_h,
                                         int64_t n_pairs, const int32_t* ia, const int32_t* ib, double* cov, int32_t launches, double* avg_ms) {
    int rc;
    if ((rc = set_device(p)) != PGO_OK) return rc;
    const int nc = (n + 63) / 64 * 64;
    std::vector<double> h((size_t)nc * nc, 0.0);
    for (int i = 0; i < nc; ++i) {
        if (i < n) std::memcpy(&h[(size_t)i * nc], a + (size_t)i * n, (size_t)n * sizeof(double));
        else h[(size_t)i * nc + i] = 1.0;
    }
    const DcParamPlan Q(nc, n / 6, sw_node, n_pairs, ia, ib);
    DBuf<double> d_a, d_scr, d_work, d_c, d_h; DBuf<int32_t> d_idx, d_fail;
    HIPCHK(p, d_a.ensure((size_t)nc * nc)); HIPCHK(p, d_scr.ensure(dense_scratch_doubles(nc))); HIPCHK(p, d_work.ensure(dense_cov_doubles(nc, Q.m, n_pairs)));
    HIPCHK(p, d_idx.ensure(dense_param_ints(Q.m, n_pairs, n_sw))); HIPCHK(p, d_fail.ensure(1));
    HIPCHK(p, d_c.ensure((size_t)std::max(n_sw, 1) * 12)); HIPCHK(p, d_h.ensure((size_t)std::max(n_sw, 1)));
    if (n_sw) {
        HIPCHK(p, hipMemcpyAsync(d_c.p, sw_c, (size_t)n_sw * 12 * sizeof(double), hipMemcpyHostToDevice, p->st));
        HIPCHK(p, hipMemcpyAsync(d_h.p, sw_h, (size_t)n_sw * sizeof(double), hipMemcpyHostToDevice, p->st));
    }
    std::vector<int32_t> staging;
    if ((rc = dense_param_upload(p, Q, n_sw, sw_node, staging, d_idx.p)) != PGO_OK) return rc;
    EventPair ev;
    HIPCHK(p, ev.create());
    float total = 0;
    int32_t fail = 0;
    for (int l = 0; l < launches && !fail; ++l) {
        HIPCHK(p, hipMemcpyAsync(d_a.p, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, p->st));
        HIPCHK(p, hipMemsetAsync(d_fail.p, 0, sizeof(int32_t), p->st));
        HIPCHK(p, hipEventRecord(ev.e0, p->st));
        if ((rc = launch_dense_param_rhs(p, nc, Q, d_work.p, d_idx.p, d_c.p, d_h.p, d_fail.p)) != PGO_OK) return rc;
        launch_dense_factor(d_a.p, nc, d_scr.p, d_fail.p, false, p->st);
        launch_dense_param_covariance(p, d_a.p, nc, Q, d_work.p, d_idx.p, d_h.p);      // (a failed factor or a refused switch row: numbers nobody reads — inside their own buffers)
        HIPCHK(p, hipEventRecord(ev.e1, p->st));
        HIPCHK(p, hipMemcpyAsync(&fail, d_fail.p, sizeof(fail), hipMemcpyDeviceToHost, p->st));
        HIPCHK(p, hipStreamSynchronize(p->st));
        float ms = 0;
        HIPCHK(p, hipEventElapsedTime(&ms, ev.e0, ev.e1));
        total += ms;
    }
    if (avg_ms) *avg_ms = (double)total / launches;
    if (fail) { p->err = std::string("matrix is not numerically positive definite") + (n_sw ? ", or a requested switch's h is not a positive finite number" : ""); return PGO_ERR_NUMERIC; }
    HIPCHK(p, hipMemcpy(cov, dense_cov_blocks(d_work.p, nc, Q.m), (size_t)36 * n_pairs * sizeof(double), hipMemcpyDeviceToHost));
    return PGO_OK;
}

int pgo_dense_spd_covariance(pgo_problem* p, int32_t n, const double* a, int64_t n_pairs, const int32_t* ia, const int32_t* ib, double* cov, int32_t launches, double* avg_ms) {
    if (!p || n <= 0 || !a || n_pairs < 1 || !ia || !ib || !cov || launches < 1) return PGO_ERR_INVALID_ARG;
    for (int64_t k = 0; k < n_pairs; ++k) if (ia[k] < 0 || ib[k] < 0 || ia[k] >= n / 6 || ib[k] >= n / 6) { p->err = "pgo_dense_spd_covariance: node index out of range (node i = rows 6 i .. 6 i + 5)"; return PGO_ERR_INVALID_ARG; }
    return dense_spd_covariance_launches(p, n, a, 0, nullptr, nullptr, nullptr, n_pairs, ia, ib, cov, launches, avg_ms);
}

int pgo_dense_spd_param_covariance(pgo_problem* p, int32_t n, const double* a, int32_t n_sw, const int32_t* sw_node, const double* sw_c, const double* sw_h,
                                   int64_t n_pairs, const int32_t* ia, const int32_t* ib, double* cov, int32_t launches, double* avg_ms) {
    if (!p || n <= 0 || !a || n_sw < 0 || (n_sw > 0 && (!sw_node || !sw_c || !sw_h)) || n_pairs < 1 || !ia || !ib || !cov || launches < 1) return PGO_ERR_INVALID_ARG;
    const int32_t nodes = n / 6;
    for (int64_t k = 0; k < n_pairs; ++k) if (ia[k] < 0 || ib[k] < 0 || ia[k] >= nodes + n_sw || ib[k] >= nodes + n_sw) { p->err = "pgo_dense_spd_param_covariance: block id out of range (node i = rows 6 i .. 6 i + 5, then n / 6 + switch)"; return PGO_ERR_INVALID_ARG; }
    for (int32_t s = 0; s < n_sw; ++s) {
        const int32_t u = sw_node[2 * s], v = sw_node[2 * s + 1];
        if (u < -1 || v < -1 || u >= nodes || v >= nodes || (u >= 0 && u == v)) { p->err = "pgo_dense_spd_param_covariance: a switch column's nodes must be distinct, below n / 6, or -1"; return PGO_ERR_INVALID_ARG; }
    }
    return dense_spd_covariance_launches(p, n, a, n_sw, sw_node, sw_c, sw_h, n_pairs, ia, ib, cov, launches, avg_ms);
}

// Diagnostic (tests): sums of squares of what this rank's cycle kernels read of level `level` (1-based) — the same whichever way the set-up ran (pgo_options.mg_dist_setup)
int pgo_mg_level_norms(pgo_problem* p, int32_t level, double* out8) {
    if (!p || !out8) return PGO_ERR_INVALID_ARG;
    for (int k = 0; k < 8; ++k) out8[k] = 0.0;
    if (!p->mg.built || p->mg.fresh_pending() || level < 1 || level > p->mg.M.n_levels || (size_t)(level - 1) >= p->mg.own.size()) { p->err = "pgo_mg_level_norms: no such level (is a hierarchy installed?)"; return PGO_ERR_INVALID_ARG; }
    int rc;
    if ((rc = set_device(p)) != PGO_OK) return rc;
    const MgLevelDev& A = p->mg.levels[level - 1];
    const OwnRange& R = p->mg.own[(size_t)level - 1];
    HIPCHK(p, hipStreamSynchronize(p->st));
    auto sq64 = [&](const double* dev, int64_t first, int64_t count, double* out) -> int {
        if (!dev || count <= 0) return PGO_OK;
        std::vector<double> h((size_t)count);
        HIPCHK(p, hipMemcpy(h.data(), dev + first, (size_t)count * sizeof(double), hipMemcpyDeviceToHost));
        long double s = 0.0L; for (double v : h) s += (long double)v * v;
        *out = (double)s; return PGO_OK;
    };
    auto sq32 = [&](const float* dev, int64_t first, int64_t count, double* out) -> int {
        if (!dev || count <= 0) return PGO_OK;
        std::vector<float> h((size_t)count);
        HIPCHK(p, hipMemcpy(h.data(), dev + first, (size_t)count * sizeof(float), hipMemcpyDeviceToHost));
        long double s = 0.0L; for (float v : h) s += (long double)v * v;
        *out = (double)s; return PGO_OK;
    };
    const bool sparse = level < p->mg.M.n_levels;
    if ((rc = sq64(A.val, R.blk0 * 36, (R.blk1 - R.blk0) * 36, out8 + 0)) != PGO_OK) return rc;
    if (sparse) {
        if ((rc = sq32(A.valf, R.blk0 * 36, (R.blk1 - R.blk0) * 36, out8 + 1)) != PGO_OK) return rc;
        if ((rc = sq64(A.Dinv, R.row0 * 36, (R.row1 - R.row0) * 36, out8 + 2)) != PGO_OK) return rc;
        if (A.smoothed && A.rt_valf) {
            if ((rc = sq32(A.rt_valf, R.w0 * 36, (R.w1 - R.w0) * 36, out8 + 3)) != PGO_OK) return rc;
            if ((rc = sq32(A.r_valf, R.rT0 * 36, (R.rT1 - R.rT0) * 36, out8 + 4)) != PGO_OK) return rc;
        }
    } else if ((rc = sq64(p->coarse.K.Ac, 0, (int64_t)p->coarse.K.nc * p->coarse.K.nc, out8 + 5)) != PGO_OK) return rc;      // the dense level: its inverse
    return PGO_OK;
}

// Test diagnostic: Z[v] = M^-1 R[v] with the asked-for preconditioner of the current LM system at `radius` (<= 0: the current one).  The system is built ONCE, the way
// pgo_apply_normal_operator builds it; then the preconditioner's operators, whatever build_system's own rules would choose for this system; then every vector takes the
// unfused start path of pcg_start: cg_init (r = R[v], z = D^-1 r) and launch_coarse_apply / mg_cycle as the PCG start launches them.  One GPU only.
int pgo_apply_preconditioner(pgo_problem* p, int32_t which, double radius, int64_t n_vec, const double* R, double* Z) {
    if (!p) return PGO_ERR_INVALID_ARG;
    auto refuse = [&](const char* why) { p->err = std::string("pgo_apply_preconditioner: ") + why; return PGO_ERR_STATE; };
    if (p->comm || p->local_ids) return refuse("one GPU only: a communicator is attached");
    if (!p->in_solve) return refuse("needs an open solve (pgo_solve_begin)");
    if (dense_mode(p)) return refuse("the dense Cholesky solver has no preconditioner");
    if (which != PGO_PRECOND_BLOCK_JACOBI && which != PGO_PRECOND_TWO_LEVEL && which != PGO_PRECOND_MULTIGRID) return refuse("invalid argument: which is not one of PGO_PRECOND_BLOCK_JACOBI / TWO_LEVEL / MULTIGRID");
    if (n_vec < 1 || !R || !Z || !std::isfinite(radius)) return refuse("invalid argument: null array, no vector, or a radius that is not finite");
    int rc;
    if ((rc = set_device(p)) != PGO_OK) return rc;
    if ((rc = mg_fresh_install(p)) != PGO_OK) return rc;      // a fresh graph's hierarchy decides which preconditioners this graph has
    ProbeRestore restore(p, radius);
    bool ok = true;
    if ((rc = build_lm_system(p, &ok)) != PGO_OK) return rc;
    if (!ok) return refuse("a diagonal block of the system is not positive definite at this radius");
    if (which == PGO_PRECOND_BLOCK_JACOBI) { p->mg.active = false; p->coarse.active = false; p->C.extra_rz = 0; }
    else if (which == PGO_PRECOND_TWO_LEVEL) {
        if (p->mg.built || !p->coarse.built) return refuse("this graph has no two-level aggregates (it has a multigrid hierarchy, or coarse_aggregates is off)");
        p->mg.active = false; p->C.extra_rz = 0;
        if ((rc = build_coarse(p, true)) != PGO_OK) return rc;
        if (!p->coarse.active) return refuse("the coarse operator of the two-level method is not positive definite at this radius");
    } else {
        if (!p->mg.built) return refuse("this graph has no multigrid hierarchy (mg_min_keyframes, or it does not coarsen)");
        p->coarse.active = false;
        if (!p->mg.active && (rc = build_mg(p)) != PGO_OK) return rc;
        if (!p->mg.active) return refuse("the multigrid operators of this system are not positive definite");
    }
    const int64_t n6 = p->N * 6;
    DBuf<double> d_in;      // the vector in b's place, and a solution vector for cg_init to zero instead of the last PCG's
    HIPCHK(p, d_in.ensure((size_t)n6 * 2));
    CgDev C = p->C;
    C.b = d_in.p; C.x = d_in.p + n6;
    std::vector<double> h((size_t)n6);
    for (int64_t v = 0; v < n_vec; ++v) {
        std::memcpy(h.data(), R + (size_t)v * n6, (size_t)n6 * sizeof(double));
        for (int64_t n = 0; n < p->N; ++n) if (!p->h_node_free[n]) for (int c = 0; c < 6; ++c) h[(size_t)n * 6 + c] = 0.0;      // rows outside the system: their residual is zero in every PCG
        HIPCHK(p, hipMemcpyAsync(d_in.p, h.data(), (size_t)n6 * sizeof(double), hipMemcpyHostToDevice, p->st));
        if (which == PGO_PRECOND_BLOCK_JACOBI) launch_cg_init(p->G, C, 0, 0.0, p->st);
        else {
            launch_cg_init_vectors(p->G, C, 0, p->st);
            if (which == PGO_PRECOND_MULTIGRID) mg_cycle(p, C, MgCycleArgs{});
            else launch_coarse_apply(p->G, C, p->coarse.K, C.r, C.z, C.part_rz, false, p->st);
        }
        double* out = Z + (size_t)v * n6;
        HIPCHK(p, hipMemcpyAsync(out, C.z, (size_t)n6 * sizeof(double), hipMemcpyDeviceToHost, p->st));
        HIPCHK(p, hipStreamSynchronize(p->st));
        for (int64_t n = 0; n < p->N; ++n) if (!p->h_node_free[n]) for (int c = 0; c < 6; ++c) out[(size_t)n * 6 + c] = 0.0;
    }
    return PGO_OK;
}

// Test diagnostic: the iterate C.x of the last PCG of the open solve, in the coordinates plus_kernel consumes
int pgo_get_linear_solution(pgo_problem* p, double* x) {
    if (!p || !x) return PGO_ERR_INVALID_ARG;
    if (p->comm || p->local_ids) { p->err = "pgo_get_linear_solution: one GPU only: a communicator is attached"; return PGO_ERR_STATE; }
    if (!p->in_solve) { p->err = "pgo_get_linear_solution needs an open solve (pgo_solve_begin)"; return PGO_ERR_STATE; }
    if (p->lm.iteration < 1) { p->err = "pgo_get_linear_solution: no PCG has run in this solve yet (pgo_lm_step)"; return PGO_ERR_STATE; }
    int rc;
    if ((rc = set_device(p)) != PGO_OK) return rc;
    return nodes_to_global(p, p->C.x, 6, x);
}

// Test diagnostic: the aggregate of every row of `level` of the installed hierarchy (level 0: the keyframes, -1 outside the system); *n = the rows of that level
int pgo_mg_level_parents(pgo_problem* p, int32_t level, int32_t* parent, int64_t capacity, int64_t* n) {
    if (!p || !n) return PGO_ERR_INVALID_ARG;
    *n = 0;
    if (p->comm || p->local_ids) { p->err = "pgo_mg_level_parents: one GPU only: a communicator is attached"; return PGO_ERR_STATE; }
    if (dense_mode(p)) { p->err = "pgo_mg_level_parents: the dense Cholesky solver builds no hierarchy"; return PGO_ERR_STATE; }
    int rc;
    if ((rc = set_device(p)) != PGO_OK) return rc;
    if (!p->graph_dirty && (rc = mg_fresh_install(p)) != PGO_OK) return rc;
    if (p->graph_dirty || !p->mg.built || p->mg.fresh_pending()) { p->err = "pgo_mg_level_parents: no hierarchy is installed (pgo_solve_begin builds it; mg_min_keyframes)"; return PGO_ERR_STATE; }
    if (level < 0 || level >= p->mg.M.n_levels) { p->err = "pgo_mg_level_parents: no such level (the coarsest level has no parents)"; return PGO_ERR_INVALID_ARG; }
    const int64_t rows = level == 0 ? p->N : (int64_t)p->mg.levels[level - 1].n;
    *n = rows;
    if (!parent) return PGO_OK;      // (size query)
    if (capacity < rows) { p->err = "pgo_mg_level_parents: the array is too short for this level"; return PGO_ERR_INVALID_ARG; }
    const int32_t* src = level == 0 ? p->mg.M.agg0 : p->mg.levels[level - 1].parent;
    HIPCHK(p, hipStreamSynchronize(p->st));
    HIPCHK(p, hipMemcpy(parent, src, (size_t)rows * sizeof(int32_t), hipMemcpyDeviceToHost));
    return PGO_OK;
}

// Test diagnostic: the matrix-free operator's workgroup tiles as the graph build uploaded them (read back from the device arrays the matvec, K2 and the record kernel walk);
// *n_tiles = 0: this handle's operator is the assembled block-CSR one
int pgo_get_matrix_free_tiles(pgo_problem* p, int32_t* tile_node0, int32_t* lanes, int32_t* pair_lanes, int32_t* first_switch_lane, int32_t* sides, int64_t capacity, int64_t* n_tiles) {
    if (!p || !n_tiles) return PGO_ERR_INVALID_ARG;
    *n_tiles = 0;
    if (p->comm || p->local_ids) { p->err = "pgo_get_matrix_free_tiles: one GPU only: a communicator is attached"; return PGO_ERR_STATE; }
    if (p->graph_dirty) { p->err = "pgo_get_matrix_free_tiles: no graph is built (pgo_solve_begin / pgo_evaluate build it)"; return PGO_ERR_STATE; }
    if (!p->built_mf) return PGO_OK;
    int rc;
    if ((rc = set_device(p)) != PGO_OK) return rc;
    const int64_t tiles = p->F.tiles;
    *n_tiles = tiles;
    if (!tile_node0 && !lanes && !pair_lanes && !first_switch_lane && !sides) return PGO_OK;      // (size query)
    if (capacity < tiles) { p->err = "pgo_get_matrix_free_tiles: the arrays are too short for this graph's tiles"; return PGO_ERR_INVALID_ARG; }
    std::vector<int32_t> node0((size_t)tiles + 1), sw0((size_t)std::max<int64_t>(tiles, 1));
    std::vector<int64_t> inc0((size_t)tiles + 1);
    std::vector<ushort4> rng((size_t)std::max<int64_t>(p->N, 1));
    HIPCHK(p, hipStreamSynchronize(p->st));
    HIPCHK(p, hipMemcpy(node0.data(), p->F.tile_node0, node0.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPCHK(p, hipMemcpy(inc0.data(), p->F.tile_inc0, inc0.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (tiles > 0) HIPCHK(p, hipMemcpy(sw0.data(), p->F.tile_sw0, (size_t)tiles * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (p->N > 0) HIPCHK(p, hipMemcpy(rng.data(), p->F.node_rng, (size_t)p->N * sizeof(ushort4), hipMemcpyDeviceToHost));
    for (int64_t t = 0; t < tiles; ++t) {
        if (tile_node0) tile_node0[t] = node0[(size_t)t];
        if (lanes) lanes[t] = (int32_t)(inc0[(size_t)t + 1] - inc0[(size_t)t]);
        if (pair_lanes) pair_lanes[t] = (int32_t)((uint32_t)sw0[(size_t)t] >> 16);
        if (first_switch_lane) first_switch_lane[t] = sw0[(size_t)t] & 0xffff;
        // the slots of a tile are numbered through its keyframes' relative-pose sides, then their switchable sides: the last keyframe's switchable range ends at the tile's side count
        const int32_t last = node0[(size_t)t + 1] - 1;
        if (sides) sides[t] = last >= node0[(size_t)t] && last < p->N ? (int32_t)rng[(size_t)last].w : 0;
    }
    if (tile_node0) tile_node0[tiles] = node0[(size_t)tiles];
    return PGO_OK;
}

// Test diagnostic: Y[v] = (H_reduced + damping) X[v] for a batch of host vectors, through the launch of pgo_apply_normal_operator, with the LM system built ONCE at `radius`
// (<= 0: the current one).  One GPU only.
int pgo_apply_normal_operator_batch(pgo_problem* p, double radius, int64_t n_vec, const double* X, double* Y) {
    if (!p) return PGO_ERR_INVALID_ARG;
    auto refuse = [&](const char* why) { p->err = std::string("pgo_apply_normal_operator_batch: ") + why; return PGO_ERR_STATE; };
    if (p->comm || p->local_ids) return refuse("one GPU only: a communicator is attached");
    if (!p->in_solve) return refuse("needs an open solve (pgo_solve_begin)");
    if (n_vec < 1 || !X || !Y || !std::isfinite(radius)) return refuse("invalid argument: null array, no vector, or a radius that is not finite");
    int rc;
    if ((rc = set_device(p)) != PGO_OK) return rc;
    ProbeRestore restore(p, radius);
    bool ok = true;
    if ((rc = build_lm_system(p, &ok)) != PGO_OK) return rc;
    const int64_t n6 = p->N * 6;
    if (n6 == 0) return PGO_OK;
    DBuf<double> d_io;
    HIPCHK(p, d_io.ensure((size_t)n6 * 2));
    for (int64_t v = 0; v < n_vec; ++v) {
        HIPCHK(p, hipMemcpyAsync(d_io.p, X + (size_t)v * n6, (size_t)n6 * sizeof(double), hipMemcpyHostToDevice, p->st));
        if (p->built_mf) launch_mf_apply(p->G, p->F, p->ScMf, p->C, d_io.p, d_io.p + n6, p->st);
        else launch_apply_operator(p->G, p->C, d_io.p, d_io.p + n6, p->st);
        HIPCHK(p, hipMemcpyAsync(Y + (size_t)v * n6, d_io.p + n6, (size_t)n6 * sizeof(double), hipMemcpyDeviceToHost, p->st));
        HIPCHK(p, hipStreamSynchronize(p->st));
    }
    return PGO_OK;
}

}  // extern "C"
