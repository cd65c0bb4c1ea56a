// pgo_solver.hip — the Ceres-compatible Levenberg-Marquardt trust-region controller of libpgo and the core of the C-ABI (include/pgo.h) around it: handle lifecycle and
// options, edge / regulariser / VIO-pose entry points, solve_begin / lm_step / solve_end, the parity hooks.  The device graph is built by pgo_graph.hip, the linear solve of
// each step is pgo_pcg.hip's, everything multi-rank pgo_shard.hip's, the measurement helpers pgo_measure.hip's.
//
// What it replaces in the reference: `ceres::Solve` (src/PoseGraphSLAM.cpp:1903) with the options at :1268-1272.  The minimiser follows
// Ceres' trust_region_minimizer.cc / levenberg_marquardt_strategy.cc control flow; the
// linear solve is a device PCG instead of SPARSE_NORMAL_CHOLESKY.  There is NO CPU fallback: without a HIP
// device pgo_create fails.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "pgo_handle.hpp"

namespace {

// K1 (+ regularisers) at state `which`; cost lands in d_scal[S_COST], d_scal[S_PRIOR_COST]
int run_k1(pgo_problem* p, int which, bool want_j) {
    int np = 0;
    launch_k1(p->G, p->d_pose[which].p, p->d_swv[which].p, want_j, part(p, 0), &np, p->st);
    if (np > 0) launch_reduce(part(p, 0), np, 0, p->d_scal.p + S_COST, p->st);
    else HIPCHK(p, hipMemsetAsync(p->d_scal.p + S_COST, 0, sizeof(double), p->st));
    launch_prior(p->G, p->d_pose[which].p, want_j, p->d_scal.p + S_PRIOR_COST, p->st);
    return PGO_OK;
}

int read_scalars(pgo_problem* p, double* h) {
    // edge-local sums [S_COST..S_SW_XNORM2] are summed over ranks; the projected-gradient norm takes the max
    // (max), the keyframe sums S_STEP2 / S_XNORM2 are owner-weighted partial sums on every rank
    int rc;
    if ((rc = allreduce(p, p->d_scal.p, 5, 0)) != PGO_OK) return rc;
    if ((rc = allreduce(p, p->d_scal.p + S_GMAX, 1, 2)) != PGO_OK) return rc;
    if ((rc = allreduce(p, p->d_scal.p + S_STEP2, 2, 0)) != PGO_OK) return rc;
    HIPCHK(p, hipMemcpyAsync(h, p->d_scal.p, S_N * sizeof(double), hipMemcpyDeviceToHost, p->st));
    HIPCHK(p, hipStreamSynchronize(p->st));
    return PGO_OK;
}

// linearise at the current state: K1 + K2 (+ all-reduce of diagonal blocks and gradient), norms
int linearize(pgo_problem* p, double* cost_out) {
    int rc;
    if ((rc = run_k1(p, p->cur, true)) != PGO_OK) return rc;
    launch_k2(p->G, p->L, !p->built_mf, p->st, p->built_mf ? &p->F : nullptr);
    ++p->lin_epoch;
    if (p->built_mf) launch_mf_compact(p->G, p->F, p->d_pose[p->cur].p, p->d_swv[p->cur].p, p->st);
    if ((rc = exchange_rows(p, p->L.Hd, 36, p->L.g, 6)) != PGO_OK) return rc;   // diagonal blocks + gradient of shared keyframes
    if (!p->scale_ready) { launch_scale_init(p->G, p->L, p->Sc, p->opt.jacobi_scaling, p->st); p->scale_ready = true; }
    int np = 0;
    launch_state_norms(p->G, p->L, p->d_pose[p->cur].p, p->d_swv[p->cur].p, part(p, 1), part(p, 2), part(p, 3), &np, p->st);
    launch_reduce(part(p, 1), np, 0, p->d_scal.p + S_XNORM2, p->st);
    launch_reduce(part(p, 2), np, 0, p->d_scal.p + S_SW_XNORM2, p->st);
    launch_reduce(part(p, 3), np, 1, p->d_scal.p + S_GMAX, p->st);
    HIPCHK(p, hipMemsetAsync(p->d_scal.p + S_MODEL, 0, 2 * sizeof(double), p->st));
    HIPCHK(p, hipMemsetAsync(p->d_scal.p + S_STEP2, 0, sizeof(double), p->st));   // not produced here; keeps the summed slot finite
    double h[S_N];
    if ((rc = read_scalars(p, h)) != PGO_OK) return rc;
    *cost_out = 0.5 * (h[S_COST] + h[S_PRIOR_COST]);
    p->lm.x_norm = std::sqrt(h[S_XNORM2] + h[S_SW_XNORM2]);
    p->lm.gmax = h[S_GMAX];
    return PGO_OK;
}

const char* step_reason_text(int r) {
    static const char* const t[] = {"ok", "REJ(rho)", "REJ(pause)", "INVALID(factorization)", "INVALID(breakdown)", "INVALID(model)", "CONVERGED"};
    return r >= 0 && r < 7 ? t[r] : "?";
}

void log_iter(pgo_problem* p, const pgo_iteration& it) {
    if (p->sum.num_logged < PGO_MAX_ITERATION_LOG) p->sum.iterations[p->sum.num_logged++] = it;
    if (p->opt.verbosity > 0)
        std::fprintf(stderr, "[pgo] it %3d cost %.12e dcost %.3e rho %.3e |step| %.3e radius %.3e cg %d (%.1e) %s %.2f ms\n", it.iteration, it.cost, it.cost_change,
                     it.relative_decrease, it.step_norm, it.trust_region_radius, it.cg_iterations, it.cg_residual, step_reason_text(it.reason), it.seconds * 1e3);
}

void terminate(pgo_problem* p, int type, const char* msg) {
    p->lm.terminated = true;
    p->sum.termination_type = type;
    std::snprintf(p->sum.message, sizeof(p->sum.message), "%s", msg);
}

int solve_begin(pgo_problem* p, const double* quat, const double* t, const double* sw, int64_t N, int64_t S) {
    if (!quat || !t || N <= 0 || S < 0 || (S > 0 && !sw)) { p->err = "null state array or bad size"; return PGO_ERR_INVALID_ARG; }
    int rc;
    if ((rc = set_device(p)) != PGO_OK) return rc;
    if (dense_mode(p)) {      // the exact dense solver: one GPU, and a matrix that fits (PGO_DENSE_MAX_KEYFRAMES)
        if (p->comm || p->local_ids) { p->err = "PGO_LINEAR_DENSE_CHOLESKY: one GPU only: a communicator is attached"; return PGO_ERR_STATE; }
        if (N > PGO_DENSE_MAX_KEYFRAMES) { p->err = "PGO_LINEAR_DENSE_CHOLESKY: more than PGO_DENSE_MAX_KEYFRAMES (" + std::to_string(PGO_DENSE_MAX_KEYFRAMES) + ") keyframes"; return PGO_ERR_INVALID_ARG; }
    }
    p->t_begin = now_s();
    if (p->mg.job.kind == MgJob::regroup) mg_drop_pending(p);
    const bool rebuild = p->graph_dirty || p->priors_dirty || N != p->N_global || S != p->S;
    if (rebuild) { if ((rc = build_graph(p, N, S, sw)) != PGO_OK) return rc; }
    else if ((rc = mg_fresh_install(p)) != PGO_OK) return rc;      // (an unchanged graph whose hierarchy no solve has needed yet: installed, then compared with this solve's start values)
    if (!rebuild && p->opt.mg_regroup_fraction > 0.0 && p->mg.built && S > 0 && sw && (int64_t)p->mg.sw_built.size() == p->swe.size()) {
        // the hierarchy of an unchanged graph was built (or regrouped inside the last solve) for other switch values than this solve starts from: the levels above level 1
        // are rebuilt for the start values whenever ANY switch differs from the record (regroup_if_moved, moved_by = 0) — a synchronous rebuild and install, tens of
        // milliseconds on C3 — so that repeated solves from the same state stay bitwise identical whatever the handle solved before.  What this costs in practice: a session's
        // next trigger has a NEW graph (one more loop edge: full rebuild anyway); only a re-solve of an unchanged graph from other switch values pays it.  (The matching
        // depends on the switch values continuously — coupling strengths order the heavy-edge matching — so "nearly the same switches" is not a safe reason to keep a hierarchy.)
        // Exception, stated: when the rebuilt hierarchy does not coarsen the one in place stays (regroup_commit) with the new switch record; the starting hierarchy then
        // depends on the handle's history.  No graph of the test suite or of profiles/ reaches that branch at a solve's start.
        if ((rc = regroup_if_moved(p, sw, false)) != PGO_OK) return rc;
    }
    // upload in the reference layout (multi-GPU: only this rank's keyframes), repack on the device
    double* io = p->d_io.p;
    const int64_t Nl = p->N;
    if (p->local_ids) { p->h_init_q.assign(quat, quat + (size_t)N * 4); p->h_init_t.assign(t, t + (size_t)N * 3); }
    if ((rc = nodes_from_global(p, quat, 4, io)) != PGO_OK) return rc;
    if ((rc = nodes_from_global(p, t, 3, io + (size_t)Nl * 4)) != PGO_OK) return rc;
    p->cur = 0;
    launch_pack_pose(io, io + (size_t)Nl * 4, p->d_pose[0].p, Nl, p->st);
    if (S > 0) {
        HIPCHK(p, hipMemcpyAsync(p->d_swv[0].p, sw, (size_t)S * sizeof(double), hipMemcpyHostToDevice, p->st));
        HIPCHK(p, hipMemcpyAsync(p->d_swv[1].p, p->d_swv[0].p, (size_t)S * sizeof(double), hipMemcpyDeviceToDevice, p->st));
    }
    HIPCHK(p, hipStreamSynchronize(p->st));
    p->t_device0 = now_s();
    std::memset(&p->sum, 0, sizeof(p->sum));
    p->in_solve = true; p->scale_ready = false; p->lm = lm_begin(p->opt);
    p->st_exchanges = p->st_allreduces = p->st_pcg_iterations = 0; p->st_bytes_neighbour = p->st_bytes_allreduce = 0.0;
    p->pcg.cg_prev_equiv = 0.0; p->pcg.cg_prev_radius = 0.0; p->mg.regroups = 0;
    if (!dense_mode(p)) two_level_solve_begin(p);      // (a dense solve leaves the two-level method's history across solves alone)
    p->sum.termination_type = PGO_NO_CONVERGENCE;
    if ((rc = linearize(p, &p->lm.x_cost)) != PGO_OK) return rc;
    p->sum.initial_cost = p->lm.x_cost;
    p->sum.final_cost = p->lm.x_cost;
    if (!std::isfinite(p->lm.x_cost)) { terminate(p, PGO_FAILURE, "initial cost is not finite"); return PGO_OK; }
    pgo_iteration it{};
    it.iteration = 0; it.step_is_valid = 1; it.step_is_successful = 1; it.cost = p->lm.x_cost; it.gradient_max_norm = p->lm.gmax; it.trust_region_radius = p->lm.radius;
    it.seconds = now_s() - p->t_device0;
    log_iter(p, it);
    return PGO_OK;
}

// candidate point x (+) delta in the other state buffer: its cost, the model cost change and the step norm
int evaluate_candidate(pgo_problem* p, LmCandidate* c) {
    const int nxt = p->cur ^ 1;
    int np = 0, np2 = 0, rc;
    launch_model_change(p->G, p->L, p->Sc, p->C.x, p->d_delta_s.p, part(p, 4), &np, p->st);
    launch_reduce(part(p, 4), np, 0, p->d_scal.p + S_MODEL, p->st);
    launch_plus(p->G, p->d_pose[p->cur].p, p->d_swv[p->cur].p, p->C.x, p->d_delta_s.p, p->d_pose[nxt].p, p->d_swv[nxt].p, part(p, 1), part(p, 2), &np2, p->st);
    launch_reduce(part(p, 1), np2, 0, p->d_scal.p + S_STEP2, p->st);
    launch_reduce(part(p, 2), np2, 0, p->d_scal.p + S_SW_STEP2, p->st);
    if ((rc = run_k1(p, nxt, false)) != PGO_OK) return rc;
    HIPCHK(p, hipMemsetAsync(p->d_scal.p + S_SW_XNORM2, 0, 2 * sizeof(double), p->st));   // SW_XNORM2, GMAX unused here
    HIPCHK(p, hipMemsetAsync(p->d_scal.p + S_XNORM2, 0, sizeof(double), p->st));
    double h[S_N] = {0};
    if ((rc = read_scalars(p, h)) != PGO_OK) return rc;
    *c = LmCandidate{0.5 * (h[S_COST] + h[S_PRIOR_COST]), -h[S_MODEL], std::sqrt(h[S_STEP2] + h[S_SW_STEP2])};
    return PGO_OK;
}

// One LM iteration: the controller's decisions (pgo_lm.hpp) around the device work — system, dense step or staged PCG, candidate, relinearisation
int lm_step(pgo_problem* p, int ignore_termination, int* done) {
    if (!p->in_solve) { p->err = "pgo_lm_step before pgo_solve_begin"; return PGO_ERR_STATE; }
    const pgo_options& o = p->opt;
    LmState& lm = p->lm;
    int rc;
    if ((rc = set_device(p)) != PGO_OK) return rc;
    if (lm.terminated && (!ignore_termination || p->sum.termination_type == PGO_FAILURE)) { *done = 1; return PGO_OK; }
    const LmStop before = lm_pre_step(lm, o, ignore_termination != 0);
    if (before.message) { terminate(p, before.type, before.message); *done = 1; return PGO_OK; }
    const double t0 = now_s();
    ++lm.iteration;
    pgo_iteration it{};
    it.iteration = lm.iteration; it.trust_region_radius = lm.radius;
    bool ok = true;
    if ((rc = build_lm_system(p, &ok)) != PGO_OK) return rc;
    double t_built = now_s();
    const bool dense = dense_mode(p);
    int why_invalid = ok ? PGO_STEP_ACCEPTED : PGO_STEP_INVALID_FACTORIZATION;      // pgo_iteration.reason of an invalid step; PGO_STEP_ACCEPTED: the linear solve is valid
    int precond_used = dense ? PGO_PRECOND_DIRECT : PGO_PRECOND_BLOCK_JACOBI;
    CgResult cg{0, false, 0.0, false};
    p->pcg.cg_extra = 0;
    LmCandidate cand{};
    bool evaluated = false;      // the step was rejected at a pause: `cand` is the candidate of that pause
    if (ok && dense) {
        // The exact solver: no PCG, no tolerance, no pause, no warm start.  Scatter + factorisation count as the system, the two sweeps as the solve; a failed pivot is
        // Ceres' linear-solver failure — the same invalid step a failed 6x6 block gives.
        if ((rc = dense_step(p, &ok, &t_built)) != PGO_OK) return rc;
        lm.have_prev_step = false;
        if (!ok) why_invalid = PGO_STEP_INVALID_FACTORIZATION;
    } else if (ok) {
        // the PCG, paused where lm_pause_plan says: at a pause the candidate is evaluated, and the same PCG resumes towards the next tolerance unless the step is clearly bad
        const LmPausePlan plan = lm_pause_plan(lm, o, p->N_global, p->pcg.cg_predicted, p->sum.num_unsuccessful_steps);
        auto tol_of = [&](int stage) { return stage < plan.n ? plan.stage[stage].tol : o.cg_rel_tolerance; };
        const bool warm = o.cg_warm_start != 0 && lm.have_prev_step && lm.reuse_diagonal;
        if ((rc = run_pcg(p, &cg, PcgPhase{tol_of(0), -1, warm})) != PGO_OK) return rc;
        for (int sidx = 0; sidx < plan.n && !cg.breakdown && !evaluated; ++sidx) {
            if ((rc = evaluate_candidate(p, &cand)) != PGO_OK) return rc;
            if (lm_clear_reject(lm, o, cand, plan.stage[sidx].reject_rho)) evaluated = true;
            else {
                const bool to_mg = p->pcg.mg_start_deferred && !p->mg.active;
                p->pcg.mg_start_deferred = false;
                if ((rc = run_pcg(p, &cg, PcgPhase{tol_of(sidx + 1), cg.iterations, false, to_mg})) != PGO_OK) return rc;
            }
        }
        if ((rc = finish_system(p, &cg, evaluated, &precond_used)) != PGO_OK) return rc;
        lm.have_prev_step = !cg.breakdown;
        if (cg.breakdown) { ok = false; why_invalid = PGO_STEP_INVALID_BREAKDOWN; }
    }
    it.cg_iterations = cg.iterations + p->pcg.cg_extra; it.cg_residual = cg.rel_residual;
    const double t_solved = now_s();
    it.seconds_system = t_built - t0; it.seconds_pcg = t_solved - t_built;
    it.cg_iterations_multigrid = p->mg.active ? cg.iterations : 0; it.single_reduction = ok && single_reduction(p) ? 1 : 0;
    if (o.verbosity > 1) std::fprintf(stderr, "[pgo] it %3d PCG: %d iterations%s after %d with block-Jacobi; system + preconditioner %.3f ms, PCG %.3f ms\n", lm.iteration, cg.iterations, p->mg.active ? " with the multigrid" : "", p->pcg.cg_extra, (t_built - t0) * 1e3, (t_solved - t_built) * 1e3);
    p->sum.cg_iterations += cg.iterations + p->pcg.cg_extra;
    if (p->mg.active) p->sum.cg_iterations_multigrid += cg.iterations;     // iterations before an in-flight switch (cg_extra) ran with block-Jacobi
    if (ok) {
        if (!evaluated && (rc = evaluate_candidate(p, &cand)) != PGO_OK) return rc;
        it.seconds_evaluate = now_s() - t_solved;
        if (o.verbosity > 1) std::fprintf(stderr, "[pgo] it %3d candidate evaluated in %.3f ms\n", lm.iteration, it.seconds_evaluate * 1e3);
    }
    it.preconditioner = precond_used;
    const LmOutcome out = lm_step_outcome(lm, o, ignore_termination != 0, why_invalid, evaluated, cand, &it);
    double new_cost = lm.x_cost;
    if (out == LmOutcome::accepted) {      // HandleSuccessfulStep: the candidate becomes the state, linearised anew
        p->cur ^= 1;
        const double t_lin = now_s();
        if ((rc = linearize(p, &new_cost)) != PGO_OK) return rc;
        it.seconds_linearize = now_s() - t_lin;
        if (o.verbosity > 1) std::fprintf(stderr, "[pgo] it %3d linearised in %.3f ms\n", lm.iteration, it.seconds_linearize * 1e3);
    }
    lm_finish_step(lm, o, out, it.relative_decrease, new_cost);
    if (out == LmOutcome::accepted) ++p->sum.num_successful_steps; else if (!it.step_is_valid || out == LmOutcome::rejected) ++p->sum.num_unsuccessful_steps;
    if (out == LmOutcome::accepted && (rc = regroup_start(p)) != PGO_OK) return rc;     // the switches have moved: does the hierarchy above level 1 still fit them?
    const LmStop after = lm_outcome_stop(out);
    if (after.message) terminate(p, after.type, after.message);
    it.cost = lm.x_cost; it.gradient_max_norm = lm.gmax; it.seconds = now_s() - t0;
    log_iter(p, it);
    p->sum.final_cost = lm.x_cost;
    *done = after.message ? 1 : 0;
    return PGO_OK;
}

int solve_end(pgo_problem* p, double* quat, double* t, double* sw, pgo_summary* out) {
    if (!p->in_solve) { p->err = "pgo_solve_end before pgo_solve_begin"; return PGO_ERR_STATE; }
    int rc;
    if ((rc = set_device(p)) != PGO_OK) return rc;
    const double t_dev = now_s();
    p->sum.num_iterations = p->lm.iteration;
    p->sum.final_cost = p->lm.x_cost;
    p->sum.seconds_device = t_dev - p->t_device0;
    if (p->sum.termination_type != PGO_FAILURE && quat && t) {
        // single write-back at the very end (reference relies on this: src/PoseGraphSLAM.cpp:1894-1903)
        double* io = p->d_io.p;
        launch_unpack_pose(p->d_pose[p->cur].p, io, io + (size_t)p->N * 4, p->N, p->st);
        const int64_t Ng = p->N_global;
        std::vector<double> hq((size_t)Ng * 4), ht((size_t)Ng * 3), hs((size_t)p->S);
        if (!p->local_ids) {
            HIPCHK(p, hipMemcpyAsync(hq.data(), io, hq.size() * sizeof(double), hipMemcpyDeviceToHost, p->st));
            HIPCHK(p, hipMemcpyAsync(ht.data(), io + (size_t)p->N * 4, ht.size() * sizeof(double), hipMemcpyDeviceToHost, p->st));
        } else {
            // every keyframe is written by its owner into a zeroed array over all keyframes; one all-reduce replicates the result
            HIPCHK(p, p->d_tmp.ensure((size_t)Ng * 7));
            HIPCHK(p, hipMemsetAsync(p->d_tmp.p, 0, (size_t)Ng * 7 * sizeof(double), p->st));
            launch_scatter_owned_pose(io, io + (size_t)p->N * 4, p->N, p->d_l2g.p, p->d_own.p, p->d_tmp.p, p->d_tmp.p + (size_t)Ng * 4, p->st);
            if ((rc = allreduce(p, p->d_tmp.p, (size_t)Ng * 7, 0)) != PGO_OK) return rc;
            HIPCHK(p, hipMemcpyAsync(hq.data(), p->d_tmp.p, hq.size() * sizeof(double), hipMemcpyDeviceToHost, p->st));
            HIPCHK(p, hipMemcpyAsync(ht.data(), p->d_tmp.p + (size_t)Ng * 4, ht.size() * sizeof(double), hipMemcpyDeviceToHost, p->st));
            HIPCHK(p, hipStreamSynchronize(p->st));
            for (int64_t g = 0; g < Ng; ++g) if (!p->h_touched_any[g]) {   // keyframes without any residual block: the values given to solve_begin
                std::copy(p->h_init_q.begin() + g * 4, p->h_init_q.begin() + g * 4 + 4, hq.begin() + g * 4); std::copy(p->h_init_t.begin() + g * 3, p->h_init_t.begin() + g * 3 + 3, ht.begin() + g * 3);
            }
        }
        if (p->S > 0) {
            if (p->local_ids) {
                // every switch is owned by the rank holding its edge: sum (owned ? value : 0) and the owner count
                std::vector<double> own((size_t)p->S * 2, 0.0), cur((size_t)p->S);
                HIPCHK(p, hipMemcpyAsync(cur.data(), p->d_swv[p->cur].p, (size_t)p->S * sizeof(double), hipMemcpyDeviceToHost, p->st));
                HIPCHK(p, hipStreamSynchronize(p->st));
                for (int64_t i = 0; i < p->S; ++i) if (p->h_sw_used[i]) { own[i] = cur[i]; own[p->S + i] = 1.0; }
                HIPCHK(p, p->d_tmp.ensure((size_t)p->S * 2));
                HIPCHK(p, hipMemcpyAsync(p->d_tmp.p, own.data(), own.size() * sizeof(double), hipMemcpyHostToDevice, p->st));
                if ((rc = allreduce(p, p->d_tmp.p, own.size(), 0)) != PGO_OK) return rc;
                HIPCHK(p, hipMemcpyAsync(own.data(), p->d_tmp.p, own.size() * sizeof(double), hipMemcpyDeviceToHost, p->st));
                HIPCHK(p, hipStreamSynchronize(p->st));
                for (int64_t i = 0; i < p->S; ++i) hs[i] = own[p->S + i] > 0.5 ? own[i] : (sw ? sw[i] : cur[i]);
            } else {
                HIPCHK(p, hipMemcpyAsync(hs.data(), p->d_swv[p->cur].p, (size_t)p->S * sizeof(double), hipMemcpyDeviceToHost, p->st));
            }
        }
        HIPCHK(p, hipStreamSynchronize(p->st));
        std::memcpy(quat, hq.data(), hq.size() * sizeof(double));
        std::memcpy(t, ht.data(), ht.size() * sizeof(double));
        if (sw && p->S > 0) std::memcpy(sw, hs.data(), hs.size() * sizeof(double));
    }
    if (!dense_mode(p)) two_level_solve_end(p);
    if (p->mg.job.kind == MgJob::regroup) mg_drop_pending(p);      // a regroup nobody needed any more: dropped (the hierarchy in place keeps its own switch record)
    if ((rc = mg_fresh_install(p)) != PGO_OK) return rc;      // a fresh graph's hierarchy that this solve never needed: installed now, for the handle's next solves
    p->sum.seconds_total = now_s() - p->t_begin;
    if (out) *out = p->sum;
    p->in_solve = false;
    return PGO_OK;
}

}  // namespace

// ================================================================================================
// C-ABI
// ================================================================================================
extern "C" {

int32_t pgo_abi_version(void) { return PGO_ABI_VERSION; }
int64_t pgo_abi_sizeof(int32_t which) { return which == 0 ? (int64_t)sizeof(pgo_options) : which == 1 ? (int64_t)sizeof(pgo_iteration) : which == 2 ? (int64_t)sizeof(pgo_summary) : 0; }

void pgo_options_init(pgo_options* o) {
    if (!o) return;
    std::memset(o, 0, sizeof(*o));
    o->mg_dist_min_rows = 8192;
    o->mg_fine_filter = 0;
    o->mg_dist_setup = 1;
    o->max_num_iterations = 10;          // src/PoseGraphSLAM.cpp:1272
    o->linear_solver = PGO_LINEAR_PCG_MATRIX_FREE;
    o->jacobi_scaling = 1;
    o->max_num_consecutive_invalid_steps = 5;
    o->initial_trust_region_radius = 1e4;
    o->max_trust_region_radius = 1e16;
    o->min_trust_region_radius = 1e-32;
    o->min_relative_decrease = 1e-3;
    o->min_lm_diagonal = 1e-6;
    o->max_lm_diagonal = 1e32;
    o->function_tolerance = 1e-6;
    o->gradient_tolerance = 1e-10;
    o->parameter_tolerance = 1e-8;
    o->cg_max_iterations = 50000;   // chain-like graphs need 5-15k iterations per step at large trust regions; capping them costs parity
    o->cg_check_every = 25;
    o->cg_warm_start = 1;
    o->cg_use_graph = 1;
    o->cg_early_tolerance = 1e-2;
    o->cg_early_reject_rho = -0.5;
    o->cg_mid_tolerance = 1e-4;
    o->cg_mid_reject_rho = -0.05;
    o->coarse_aggregates = 768;
    o->coarse_min_radius = 1e7;
    o->mg_min_keyframes = 5000;
    o->mg_min_keyframes_switchable = 5000;
    o->mg_omega = 0.9;
    o->mg_correction_scale = 1.0;
    o->mg_first_passes = 3;
    o->mg_passes = 0;
    o->mg_dense_max_nodes = 512;
    o->mg_switch_iterations = 400;
    o->mg_loop_discount = 3.0;
    o->mg_regroup_fraction = 0.02;
    o->mg_prolongation_damping = 0.6;
    o->mg_smoothed_levels = -1;
    o->cg_rel_tolerance = 3e-10;    // keeps the 10-iteration chi^2 of C3 within 1e-8 of the independent CPU trajectory whatever the preconditioner schedule (1e-9: 1e-7)
    o->device_id = -1;
    o->verbosity = 0;
    o->cg_single_reduction = 1;
    o->cg_pause_always = 0;
    o->mg_smoothed_fine = -1;
    o->mg_explicit_transfer = 1;
    o->cg_end_game = 1;
}

int pgo_create(pgo_problem** out, const pgo_options* opts) {
    if (!out) return PGO_ERR_INVALID_ARG;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return PGO_ERR_NO_DEVICE;
    pgo_problem* p = new (std::nothrow) pgo_problem();
    if (!p) return PGO_ERR_OUT_OF_MEMORY;
    if (opts) p->opt = *opts; else pgo_options_init(&p->opt);
    int dev = p->opt.device_id;
    if (dev < 0) { if (hipGetDevice(&dev) != hipSuccess) dev = 0; }
    if (dev >= count) { delete p; return PGO_ERR_NO_DEVICE; }
    p->device = dev;
    if (hipSetDevice(dev) != hipSuccess || hipStreamCreateWithFlags(&p->st.s, hipStreamNonBlocking) != hipSuccess) { delete p; return PGO_ERR_NO_DEVICE; }
    std::memset(&p->sum, 0, sizeof(p->sum));
    if (p->pcg.create() != hipSuccess) { delete p; return PGO_ERR_OUT_OF_MEMORY; }
    // One-time costs of the process belong here, not in the first trigger: the first device allocation and the first kernel launch of the library (its code object goes to the
    // device).  Failures here are not errors (the solve reports its own).  (A captured + instantiated graph would also take the first hipGraphInstantiate of the process off the
    // first long PCG — 9.4 ms against 0.2 ms for later ones — but a capture in one thread makes a concurrent synchronous hipMemcpy of ANOTHER thread fail with
    // hipErrorStreamCaptureImplicit on this runtime, thread-local mode or not: handles are created concurrently by callers that run one rank per thread.)
    {
        double* w = nullptr;
        if (hipMalloc((void**)&w, 4096) == hipSuccess) {
            (void)hipMemsetAsync(w, 0, 4096, p->st);
            launch_reduce(w, 0, 0, w + 8, p->st);
            (void)hipStreamSynchronize(p->st);
            (void)hipFree(w);
            // the runtime's copy paths by size class (pageable host memory, both directions) set up their staging on first use: measured, the first wake-up of a session
            // 27.3 -> 19.6 ms with these copies done here
            double* big = nullptr;
            if (hipMalloc((void**)&big, (size_t)4 << 20) == hipSuccess) {
                std::vector<char> host((size_t)4 << 20, 0);
                for (size_t bytes : {(size_t)1 << 10, (size_t)16 << 10, (size_t)32 << 10, (size_t)64 << 10, (size_t)256 << 10, (size_t)1 << 20, (size_t)4 << 20}) {
                    (void)hipMemcpyAsync(big, host.data(), bytes, hipMemcpyHostToDevice, p->st);
                    (void)hipMemcpyAsync(host.data(), big, bytes, hipMemcpyDeviceToHost, p->st);
                    (void)hipStreamSynchronize(p->st);
                }
                (void)hipFree(big);
            }
            (void)hipGetLastError();
        }
    }
    *out = p;
    return PGO_OK;
}

int pgo_destroy(pgo_problem* p) {
    if (!p) return PGO_ERR_INVALID_ARG;
    mg_drop_pending(p);
    (void)hipSetDevice(p->device);
    // (the in-process group's peers may be gone: the group is aborted, not waited for.  Known limit: the send buffers are freed with the handle, once its stream has drained —
    // on one GPU hipFree waits for the peers' kernels as well, across GPUs a peer's copy kernel of the last exchange could still be reading them)
    if (p->comm) p->comm->abandon();
    p->comm.reset();
    (void)hipStreamSynchronize(p->st);
    delete p;      // (its members release the captured graphs, the pinned poll buffer and its events, then the stream, then the device buffers)
    return PGO_OK;
}

int pgo_set_options(pgo_problem* p, const pgo_options* o) {
    if (!p || !o) return PGO_ERR_INVALID_ARG;
    const int dev = p->opt.device_id;
    mg_drop_pending(p);
    if (o->linear_solver != p->opt.linear_solver) p->graph_dirty = true;
    // the preconditioner hierarchies are part of the device graph build
    if (o->mg_min_keyframes != p->opt.mg_min_keyframes || o->mg_min_keyframes_switchable != p->opt.mg_min_keyframes_switchable || o->mg_first_passes != p->opt.mg_first_passes || o->mg_passes != p->opt.mg_passes ||
        o->mg_dense_max_nodes != p->opt.mg_dense_max_nodes || o->coarse_aggregates != p->opt.coarse_aggregates || o->mg_smoothed_levels != p->opt.mg_smoothed_levels || o->mg_loop_discount != p->opt.mg_loop_discount ||
        o->mg_explicit_transfer != p->opt.mg_explicit_transfer || o->mg_smoothed_fine != p->opt.mg_smoothed_fine || o->mg_dist_min_rows != p->opt.mg_dist_min_rows || o->mg_dist_setup != p->opt.mg_dist_setup ||
        o->mg_fine_filter != p->opt.mg_fine_filter) p->graph_dirty = true;
    p->opt = *o;
    p->opt.device_id = dev;   // the device binding is fixed at create
    return PGO_OK;
}

int pgo_reserve(pgo_problem* p, int64_t n_nodes, int64_t n_edges) {
    if (!p || n_nodes < 0 || n_edges < 0) return PGO_ERR_INVALID_ARG;
    if ((size_t)n_edges <= p->rel.c1.capacity() && (size_t)n_edges <= p->rel.c2.capacity() && (size_t)n_edges * 8 <= p->rel.meas.capacity()) return PGO_OK;      // nothing moves
    // the edge arrays are about to be reallocated: the hierarchy workers (a fresh graph's, a regroup's) read them — same rule as every other mutating entry point
    if (p->in_solve) { p->err = "pgo_reserve inside a solve (between pgo_solve_begin and pgo_solve_end)"; return PGO_ERR_STATE; }
    mg_drop_pending(p);
    p->rel.c1.reserve(n_edges); p->rel.c2.reserve(n_edges); p->rel.meas.reserve((size_t)n_edges * 8);
    return PGO_OK;
}

int pgo_add_relpose_edges(pgo_problem* p, int64_t n, const int32_t* c1, const int32_t* c2, const double* T, const double* w) {
    if (!p) return PGO_ERR_INVALID_ARG;
    if (n > 0 && !w) { p->err = "weight array required for relative-pose edges"; return PGO_ERR_INVALID_ARG; }
    return add_edges(p, p->rel, n, c1, c2, T, w, nullptr);
}
int pgo_add_relpose_edges_robust(pgo_problem* p, int64_t n, const int32_t* c1, const int32_t* c2, const double* T, const double* w, int32_t loss, double loss_a) {
    if (!p) return PGO_ERR_INVALID_ARG;
    if (loss != PGO_LOSS_TRIVIAL && loss != PGO_LOSS_HUBER && loss != PGO_LOSS_CAUCHY) { p->err = "unknown robust loss"; return PGO_ERR_INVALID_ARG; }
    if (loss != PGO_LOSS_TRIVIAL && !(std::isfinite(loss_a) && loss_a > 0.0)) { p->err = "the robust loss parameter must be finite and positive"; return PGO_ERR_INVALID_ARG; }
    if (n > 0 && !w) { p->err = "weight array required for relative-pose edges"; return PGO_ERR_INVALID_ARG; }
    return add_edges(p, p->rel, n, c1, c2, T, w, nullptr, loss == PGO_LOSS_HUBER ? loss_a : loss == PGO_LOSS_CAUCHY ? -loss_a : 0.0);
}
int pgo_get_relpose_edge_loss(const pgo_problem* p, int64_t first, int64_t n, int32_t* loss, double* loss_a) {
    if (!p || first < 0 || n < 0 || first + n > p->rel.size()) return PGO_ERR_INVALID_ARG;
    for (int64_t k = 0; k < n; ++k) {
        const double enc = first + k < (int64_t)p->rel.loss.size() ? p->rel.loss[first + k] : 0.0;
        if (loss) loss[k] = enc > 0.0 ? PGO_LOSS_HUBER : enc < 0.0 ? PGO_LOSS_CAUCHY : PGO_LOSS_TRIVIAL;
        if (loss_a) loss_a[k] = std::fabs(enc);
    }
    return PGO_OK;
}
int pgo_add_switchable_edges(pgo_problem* p, int64_t n, const int32_t* c1, const int32_t* c2, const double* T, const double* w, const int32_t* sw) {
    if (!p) return PGO_ERR_INVALID_ARG;
    if (n > 0 && !sw) { p->err = "switch index array required"; return PGO_ERR_INVALID_ARG; }
    return add_edges(p, p->swe, n, c1, c2, T, w, sw);
}
int pgo_add_switchable_edges_robust(pgo_problem* p, int64_t n, const int32_t* c1, const int32_t* c2, const double* T, const double* w, const int32_t* sw, int32_t loss, double loss_a) {
    if (!p) return PGO_ERR_INVALID_ARG;
    if (loss != PGO_LOSS_TRIVIAL && loss != PGO_LOSS_HUBER && loss != PGO_LOSS_CAUCHY) { p->err = "unknown robust loss"; return PGO_ERR_INVALID_ARG; }
    if (loss != PGO_LOSS_TRIVIAL && !(std::isfinite(loss_a) && loss_a > 0.0)) { p->err = "the robust loss parameter must be finite and positive"; return PGO_ERR_INVALID_ARG; }
    if (n > 0 && !sw) { p->err = "switch index array required"; return PGO_ERR_INVALID_ARG; }
    return add_edges(p, p->swe, n, c1, c2, T, w, sw, loss == PGO_LOSS_HUBER ? loss_a : loss == PGO_LOSS_CAUCHY ? -loss_a : 0.0);
}
int pgo_get_switchable_edge_loss(const pgo_problem* p, int64_t first, int64_t n, int32_t* loss, double* loss_a) {
    if (!p || first < 0 || n < 0 || first + n > p->swe.size()) return PGO_ERR_INVALID_ARG;
    for (int64_t k = 0; k < n; ++k) {
        const double enc = first + k < (int64_t)p->swe.loss.size() ? p->swe.loss[first + k] : 0.0;
        if (loss) loss[k] = enc > 0.0 ? PGO_LOSS_HUBER : enc < 0.0 ? PGO_LOSS_CAUCHY : PGO_LOSS_TRIVIAL;
        if (loss_a) loss_a[k] = std::fabs(enc);
    }
    return PGO_OK;
}
int pgo_set_node_regularizers(pgo_problem* p, int64_t n, const int32_t* node, const double* target, const double* weight) {
    if (!p || n < 0 || (n > 0 && (!node || !target || !weight))) return PGO_ERR_INVALID_ARG;
    std::vector<PriorDev> v((size_t)n);
    for (int64_t k = 0; k < n; ++k) {
        if (node[k] < 0) { p->err = "negative regulariser node"; return PGO_ERR_INVALID_ARG; }
        const double* T = target + 16 * k;
        PriorDev& P = v[k];
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) P.Rf[r * 3 + c] = T[c * 4 + r];
        P.tf[0] = T[12]; P.tf[1] = T[13]; P.tf[2] = T[14];
        eigen_matrix_to_quat(P.Rf, P.qf);
        P.w = weight[k]; P.node = node[k]; P.pad_ = 0;
    }
    mg_drop_pending(p);
    p->priors.swap(v);
    p->priors_dirty = true;
    return PGO_OK;
}
int pgo_set_nodes_constant(pgo_problem* p, int64_t n, const int32_t* node) {
    if (!p || n < 0 || (n > 0 && !node)) return PGO_ERR_INVALID_ARG;
    for (int64_t k = 0; k < n; ++k) if (node[k] < 0) return PGO_ERR_INVALID_ARG;
    mg_drop_pending(p);      // (the worker reads h_node_free / constant_nodes)
    p->constant_nodes.insert(p->constant_nodes.end(), node, node + n);
    p->graph_dirty = true;
    return PGO_OK;
}
// ---- graph construction from the resident VIO poses (K0) ----
int pgo_set_vio_poses(pgo_problem* p, int64_t first, int64_t n, const double* w_M) {
    if (!p || first < 0 || n < 0 || (n > 0 && !w_M)) return PGO_ERR_INVALID_ARG;
    if (first > p->n_vio) { p->err = "VIO poses must be appended contiguously"; return PGO_ERR_INVALID_ARG; }
    if (n == 0) return PGO_OK;
    HIPCHK(p, hipSetDevice(p->device));
    const int64_t need = first + n;
    if ((size_t)need * 16 > p->d_vio.cap) {       // grow geometrically, keep the old poses
        DBuf<double> bigger;
        HIPCHK(p, bigger.ensure((size_t)std::max<int64_t>(need + need / 2, 1024) * 16));
        if (p->n_vio > 0) HIPCHK(p, hipMemcpyAsync(bigger.p, p->d_vio.p, (size_t)p->n_vio * 16 * sizeof(double), hipMemcpyDeviceToDevice, p->st));
        HIPCHK(p, hipStreamSynchronize(p->st));
        std::swap(p->d_vio.p, bigger.p); std::swap(p->d_vio.cap, bigger.cap);
    }
    HIPCHK(p, hipMemcpyAsync(p->d_vio.p + (size_t)first * 16, w_M, (size_t)n * 16 * sizeof(double), hipMemcpyHostToDevice, p->st));
    HIPCHK(p, hipStreamSynchronize(p->st));
    p->n_vio = std::max(p->n_vio, need);
    return PGO_OK;
}
int pgo_num_vio_poses(const pgo_problem* p, int64_t* n) { if (!p || !n) return PGO_ERR_INVALID_ARG; *n = p->n_vio; return PGO_OK; }

int pgo_add_odometry_edges_from_vio(pgo_problem* p, const int32_t* set_id, int64_t u_begin, int64_t u_end, int32_t f_max, int32_t use_yaw_weight, int64_t* n_added) {
    if (!p || u_begin < 0 || u_end < u_begin || f_max < 1) return PGO_ERR_INVALID_ARG;
    if (u_end > p->n_vio) { p->err = "odometry edges requested beyond the resident VIO poses"; return PGO_ERR_INVALID_ARG; }
    if (p->in_solve) { p->err = "graph construction inside a solve"; return PGO_ERR_STATE; }
    mg_drop_pending(p);      // (a regroup's worker left behind by a failed solve reads the edge lists)
    std::vector<int32_t> c1, c2;
    c1.reserve((size_t)(u_end - u_begin) * f_max); c2.reserve(c1.capacity());
    for (int64_t u = u_begin; u < u_end; ++u)
        for (int f = 1; f <= f_max; ++f) {
            if (u - f < 0) continue;                                           // (:1588-1591)
            if (set_id && (set_id[u] < 0 || set_id[u - f] < 0)) continue;      // dead zone (:1583-1586)
            c1.push_back((int32_t)u); c2.push_back((int32_t)(u - f));
        }
    const int64_t n = (int64_t)c1.size();
    if (n_added) *n_added = n;
    if (n == 0) return PGO_OK;
    HIPCHK(p, hipSetDevice(p->device));
    DBuf<int32_t>& d_c = p->d_vio_idx;            // c1 then c2 (kept across calls)
    DBuf<double>& d_meas = p->d_vio_meas;
    HIPCHK(p, d_c.ensure((size_t)2 * n)); HIPCHK(p, d_meas.ensure((size_t)8 * n));
    HIPCHK(p, hipMemcpyAsync(d_c.p, c1.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, p->st));
    HIPCHK(p, hipMemcpyAsync(d_c.p + n, c2.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, p->st));
    launch_vio_odometry(n, d_c.p, d_c.p + n, p->d_vio.p, use_yaw_weight, d_meas.p, p->st);
    HostClass& H = p->rel;
    const size_t base = H.c1.size();
    H.meas.resize((base + n) * 8);
    // (the second wake-up of a process spends ~8 ms inside this copy call — runtime-internal, once; a pinned staging buffer of our own does not change it: measured)
    HIPCHK(p, hipMemcpyAsync(&H.meas[base * 8], d_meas.p, (size_t)8 * n * sizeof(double), hipMemcpyDeviceToHost, p->st));
    const hipError_t e = hipStreamSynchronize(p->st);
    if (e != hipSuccess) { H.meas.resize(base * 8); p->err = hipGetErrorString(e); return PGO_ERR_HIP; }
    H.c1.insert(H.c1.end(), c1.begin(), c1.end());
    H.c2.insert(H.c2.end(), c2.begin(), c2.end());
    p->graph_dirty = true;
    return PGO_OK;
}

int pgo_initial_guess_from_vio(pgo_problem* p, int64_t n_left, const double* left, const int32_t* left_of_node, int64_t u_begin, int64_t u_end, double* quat, double* t) {
    if (!p || n_left < 0 || u_begin < 0 || u_end < u_begin) return PGO_ERR_INVALID_ARG;
    const int64_t cnt = u_end - u_begin;
    if (cnt == 0) return PGO_OK;
    if (!left_of_node || !quat || !t || (n_left > 0 && !left)) return PGO_ERR_INVALID_ARG;
    if (u_end > p->n_vio) { p->err = "initial guesses requested beyond the resident VIO poses"; return PGO_ERR_INVALID_ARG; }
    bool any = false;
    for (int64_t i = 0; i < cnt; ++i) {
        if (left_of_node[i] >= n_left) { p->err = "left-matrix selector out of range"; return PGO_ERR_INVALID_ARG; }
        any |= left_of_node[i] >= 0;
    }
    if (!any) return PGO_OK;
    HIPCHK(p, hipSetDevice(p->device));
    DBuf<double> d_left, d_q, d_t;
    DBuf<int32_t> d_sel;
    HIPCHK(p, d_left.ensure((size_t)n_left * 16)); HIPCHK(p, d_q.ensure((size_t)cnt * 4)); HIPCHK(p, d_t.ensure((size_t)cnt * 3)); HIPCHK(p, d_sel.ensure((size_t)cnt));
    HIPCHK(p, hipMemcpyAsync(d_left.p, left, (size_t)n_left * 16 * sizeof(double), hipMemcpyHostToDevice, p->st));
    HIPCHK(p, hipMemcpyAsync(d_sel.p, left_of_node, (size_t)cnt * sizeof(int32_t), hipMemcpyHostToDevice, p->st));
    // untouched keyframes keep the caller's values: seed the staging buffers with them
    HIPCHK(p, hipMemcpyAsync(d_q.p, quat + u_begin * 4, (size_t)cnt * 4 * sizeof(double), hipMemcpyHostToDevice, p->st));
    HIPCHK(p, hipMemcpyAsync(d_t.p, t + u_begin * 3, (size_t)cnt * 3 * sizeof(double), hipMemcpyHostToDevice, p->st));
    launch_vio_initial_guess(u_begin, cnt, d_left.p, d_sel.p, p->d_vio.p, d_q.p, d_t.p, p->st);
    HIPCHK(p, hipMemcpyAsync(quat + u_begin * 4, d_q.p, (size_t)cnt * 4 * sizeof(double), hipMemcpyDeviceToHost, p->st));
    HIPCHK(p, hipMemcpyAsync(t + u_begin * 3, d_t.p, (size_t)cnt * 3 * sizeof(double), hipMemcpyDeviceToHost, p->st));
    HIPCHK(p, hipStreamSynchronize(p->st));
    return PGO_OK;
}

int pgo_get_relpose_edge_records(const pgo_problem* p, int64_t first, int64_t n, int32_t* c1, int32_t* c2, double* record8) {
    if (!p || first < 0 || n < 0 || first + n > p->rel.size()) return PGO_ERR_INVALID_ARG;
    if (c1) std::copy(p->rel.c1.begin() + first, p->rel.c1.begin() + first + n, c1);
    if (c2) std::copy(p->rel.c2.begin() + first, p->rel.c2.begin() + first + n, c2);
    if (record8) std::copy(p->rel.meas.begin() + first * 8, p->rel.meas.begin() + (first + n) * 8, record8);
    return PGO_OK;
}
int pgo_num_relpose_edges(const pgo_problem* p, int64_t* n) { if (!p || !n) return PGO_ERR_INVALID_ARG; *n = p->rel.size(); return PGO_OK; }
int pgo_num_switchable_edges(const pgo_problem* p, int64_t* n) { if (!p || !n) return PGO_ERR_INVALID_ARG; *n = p->swe.size(); return PGO_OK; }
int pgo_num_regularizers(const pgo_problem* p, int64_t* n) { if (!p || !n) return PGO_ERR_INVALID_ARG; *n = (int64_t)p->priors.size(); return PGO_OK; }

int pgo_solve_begin(pgo_problem* p, const double* q, const double* t, const double* sw, int64_t N, int64_t S) {
    if (!p) return PGO_ERR_INVALID_ARG;
    return solve_begin(p, q, t, sw, N, S);
}
// a failed step or write-back: no regroup worker outlives it (it reads host arrays the caller may change next), and a stream capture a failing launch left open is ended
static void after_failure(pgo_problem* p) {
    mg_drop_pending(p);
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (p->st && hipStreamIsCapturing(p->st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) { hipGraph_t g = nullptr; (void)hipStreamEndCapture(p->st, &g); if (g) (void)hipGraphDestroy(g); p->pcg.cg_graph_failed = true; }
    (void)hipGetLastError();
}
int pgo_lm_step(pgo_problem* p, int32_t ignore_termination, int32_t* done) {
    if (!p) return PGO_ERR_INVALID_ARG;
    int d = 0;
    const int rc = lm_step(p, ignore_termination, &d);
    if (rc != PGO_OK) after_failure(p);
    if (done) *done = d;
    return rc;
}
int pgo_solve_end(pgo_problem* p, double* q, double* t, double* sw, pgo_summary* s) {
    if (!p) return PGO_ERR_INVALID_ARG;
    const int rc = solve_end(p, q, t, sw, s);
    if (rc != PGO_OK) { after_failure(p); p->in_solve = false; }
    return rc;
}
int pgo_solve(pgo_problem* p, double* q, double* t, double* sw, int64_t N, int64_t S, pgo_summary* s) {
    if (!p) return PGO_ERR_INVALID_ARG;
    int rc = solve_begin(p, q, t, sw, N, S);
    if (rc != PGO_OK) return rc;
    int done = p->lm.terminated ? 1 : 0;
    while (!done) { rc = lm_step(p, 0, &done); if (rc != PGO_OK) { after_failure(p); p->in_solve = false; return rc; } }
    rc = solve_end(p, q, t, sw, s);
    if (rc != PGO_OK) { after_failure(p); p->in_solve = false; }
    return rc;
}

int pgo_evaluate(pgo_problem* p, const double* q, const double* t, const double* sw, int64_t N, int64_t S, double* cost, double* residuals, double* gradient) {
    if (!p) return PGO_ERR_INVALID_ARG;
    const pgo_summary keep = p->sum;
    int rc = solve_begin(p, q, t, sw, N, S);   // upload + K1 + K2 + norms at the given point
    if (rc != PGO_OK) return rc;
    p->in_solve = false;
    if (cost) *cost = p->lm.x_cost;
    const int64_t Er = p->G.rel.E, Es = p->G.sw.E, Eg = p->G.n_prior;
    if (residuals) {
        const int64_t total = 6 * Er + 7 * Es + 6 * Eg;
        HIPCHK(p, p->d_tmp.ensure(std::max<int64_t>(total, 1)));
        launch_unpack_k1(p->G, 0, 0, Er, p->d_tmp.p, nullptr, nullptr, nullptr, p->st);
        launch_unpack_k1(p->G, 1, 0, Es, p->d_tmp.p + 6 * Er, nullptr, nullptr, nullptr, p->st);
        launch_unpack_k1(p->G, 2, 0, Eg, p->d_tmp.p + 6 * Er + 7 * Es, nullptr, nullptr, nullptr, p->st);
        HIPCHK(p, hipMemcpyAsync(residuals, p->d_tmp.p, total * sizeof(double), hipMemcpyDeviceToHost, p->st));
        HIPCHK(p, hipStreamSynchronize(p->st));
    }
    if (gradient) {
        std::vector<double> gs((size_t)std::max<int64_t>(Es, 1));
        // constant keyframes have no gradient entry; zero them on the device copy before it is spread over all keyframes
        std::vector<double> gl((size_t)p->N * 6);
        HIPCHK(p, hipMemcpyAsync(gl.data(), p->L.g, gl.size() * sizeof(double), hipMemcpyDeviceToHost, p->st));
        if (Es) HIPCHK(p, hipMemcpyAsync(gs.data(), p->L.gs, Es * sizeof(double), hipMemcpyDeviceToHost, p->st));
        HIPCHK(p, hipStreamSynchronize(p->st));
        for (int64_t n = 0; n < p->N; ++n) if (!p->h_node_free[n]) for (int c = 0; c < 6; ++c) gl[6 * n + c] = 0.0;
        HIPCHK(p, p->d_io.ensure(gl.size()));
        HIPCHK(p, hipMemcpyAsync(p->d_io.p, gl.data(), gl.size() * sizeof(double), hipMemcpyHostToDevice, p->st));
        if ((rc = nodes_to_global(p, p->d_io.p, 6, gradient)) != PGO_OK) return rc;
        for (int64_t i = 0; i < S; ++i) gradient[6 * N + i] = 0.0;
        for (int64_t e = 0; e < Es; ++e) gradient[6 * N + p->swe.sw[e]] = gs[e];   // multi-GPU: each rank reports the switches of its own edges
    }
    p->sum = keep;
    return PGO_OK;
}

// The covariance blocks of pgo_pose_covariance and pgo_covariance (the contracts: include/pgo.h; the algebra: csrc/pgo_dense_math.hpp).  The handle is linearised at the
// given point the way pgo_evaluate does it, and everything that carries over to the next solve is put back: the summary, the LM controller's state and the two-level
// method's history across solves (solve_begin spends one solve of its back-off).  name: the entry point, for its messages.  pose_only (pgo_pose_covariance): ids at or
// above N are out of range, and a handle without block-CSR values is refused — by its option before the graph is looked at, by its graph build after solve_begin.
static int covariance_blocks(pgo_problem* p, const char* name, bool pose_only, const double* q, const double* t, const double* sw, int64_t N, int64_t S, int64_t n_pairs,
                             const int32_t* block_a, const int32_t* block_b, double* cov) {
    if (!p) return PGO_ERR_INVALID_ARG;
    const std::string who = name;
    if (n_pairs < 0 || (n_pairs > 0 && (!block_a || !block_b || !cov))) { p->err = who + ": null pair array or negative count"; return PGO_ERR_INVALID_ARG; }
    if (p->in_solve) { p->err = who + " inside a solve (between pgo_solve_begin and pgo_solve_end)"; return PGO_ERR_STATE; }
    if (p->comm || p->local_ids) { p->err = who + ": one GPU only: a communicator is attached"; return PGO_ERR_STATE; }
    if (pose_only && p->opt.linear_solver == PGO_LINEAR_PCG_MATRIX_FREE) {
        p->err = who + ": pgo_options.linear_solver = PGO_LINEAR_PCG_MATRIX_FREE keeps no block-CSR values to factor; select PGO_LINEAR_PCG_BLOCK_JACOBI or PGO_LINEAR_DENSE_CHOLESKY";
        return PGO_ERR_STATE;
    }
    if (N > PGO_DENSE_MAX_KEYFRAMES) { p->err = who + ": more than PGO_DENSE_MAX_KEYFRAMES (" + std::to_string(PGO_DENSE_MAX_KEYFRAMES) + ") keyframes"; return PGO_ERR_INVALID_ARG; }
    if (N < 0 || S < 0) { p->err = who + ": negative count"; return PGO_ERR_INVALID_ARG; }
    std::vector<uint8_t> referenced((size_t)N, 0);
    auto mark = [&](int32_t n) { if (n >= 0 && n < N) referenced[(size_t)n] = 1; };
    for (const HostClass* H : {&p->rel, &p->swe}) for (int64_t e = 0; e < H->size(); ++e) { mark(H->c1[e]); mark(H->c2[e]); }
    for (const PriorDev& pr : p->priors) mark(pr.node);
    std::vector<int32_t> edge_of((size_t)S, -1);      // caller's switch index -> internal index of the switchable edge that uses it
    for (int64_t e = 0; e < p->swe.size(); ++e) if (p->swe.sw[e] >= 0 && p->swe.sw[e] < S) edge_of[(size_t)p->swe.sw[e]] = (int32_t)e;
    for (int64_t k = 0; k < n_pairs; ++k) for (int32_t id : {block_a[k], block_b[k]}) {
        if (id < 0 || id >= (pose_only ? N : N + S)) {
            p->err = who + (pose_only ? ": keyframe index out of range" : ": block id out of range (keyframes 0 .. n_nodes - 1, then n_nodes + switch index)");
            return PGO_ERR_INVALID_ARG;
        }
        if (id < N && !referenced[(size_t)id]) { p->err = who + ": keyframe " + std::to_string(id) + " is referenced by no residual block: it has no covariance"; return PGO_ERR_INVALID_ARG; }
        if (id >= N && edge_of[(size_t)(id - N)] < 0) { p->err = who + ": switch " + std::to_string(id - N) + " is used by no switchable edge: it has no covariance"; return PGO_ERR_INVALID_ARG; }
    }
    struct Restore {      // (dense mode: solve_begin leaves the history alone, and a graph build for the exact solver resets it on purpose)
        pgo_problem* p; pgo_summary sum; LmState lm; CoarseState::History hist;
        ~Restore() { p->in_solve = false; p->sum = sum; p->lm = lm; if (!dense_mode(p)) p->coarse.hist = hist; }
    } restore{p, p->sum, p->lm, p->coarse.hist};
    int rc = solve_begin(p, q, t, sw, N, S);   // upload + K1 + K2 at the given point (a changed graph is built here, for the handle's own linear solver)
    if (rc != PGO_OK) return rc;
    if (!std::isfinite(p->lm.x_cost)) { p->err = who + ": the cost at this point is not finite"; return PGO_ERR_NUMERIC; }
    if (pose_only && p->built_mf) { p->err = who + ": the graph was built matrix-free"; return PGO_ERR_STATE; }
    // pairs with a constant keyframe: zero blocks (constant keyframes are not parameters), filled in here; the others go to the device with keyframe ids as they are and
    // switch ids by internal edge index
    auto is_free = [&](int32_t n) { return p->h_node_free[(size_t)n] != 0; };
    std::vector<int32_t> ia, ib; std::vector<int64_t> where;
    for (int64_t k = 0; k < n_pairs; ++k) {
        const int32_t a = block_a[k], b = block_b[k];
        if ((a < N && !is_free(a)) || (b < N && !is_free(b))) continue;
        ia.push_back(a < N ? a : (int32_t)N + edge_of[(size_t)(a - N)]); ib.push_back(b < N ? b : (int32_t)N + edge_of[(size_t)(b - N)]); where.push_back(k);
    }
    std::vector<double> blocks(ia.size() * 36);
    if (!ia.empty()) {
        std::vector<int32_t> sw_node((size_t)p->swe.size() * 2);      // a constant endpoint drops its side of c_e
        for (int64_t e = 0; e < p->swe.size(); ++e) { sw_node[2 * (size_t)e] = is_free(p->swe.c1[e]) ? p->swe.c1[e] : -1; sw_node[2 * (size_t)e + 1] = is_free(p->swe.c2[e]) ? p->swe.c2[e] : -1; }
        bool ok = true;
        if ((rc = dense_param_covariance(p, sw_node, (int64_t)ia.size(), ia.data(), ib.data(), blocks.data(), &ok)) != PGO_OK) { after_failure(p); return rc; }
        if (!ok) {
            p->err = who + ": the undamped system is not numerically positive definite (is the gauge fixed: a regulariser or a constant keyframe?)" +
                     (pose_only ? "" : ", or a requested switch's J_s^T J_s is not a positive finite number");
            return PGO_ERR_NUMERIC;
        }
    }
    std::fill(cov, cov + (size_t)n_pairs * 36, 0.0);
    for (size_t u = 0; u < where.size(); ++u) std::memcpy(cov + (size_t)where[u] * 36, blocks.data() + u * 36, 36 * sizeof(double));
    return PGO_OK;
}

// Marginal covariances of keyframe poses (ceres::Covariance::Compute + GetCovarianceBlockInTangentSpace for pose blocks), on a handle that keeps block-CSR values
int pgo_pose_covariance(pgo_problem* p, const double* q, const double* t, const double* sw, int64_t N, int64_t S, int64_t n_pairs, const int32_t* node_a, const int32_t* node_b, double* cov) {
    return covariance_blocks(p, "pgo_pose_covariance", true, q, t, sw, N, S, n_pairs, node_a, node_b, cov);
}

// Covariance blocks of pose AND switch parameter blocks, on every kind of graph build
int pgo_covariance(pgo_problem* p, const double* q, const double* t, const double* sw, int64_t N, int64_t S, int64_t n_pairs, const int32_t* block_a, const int32_t* block_b, double* cov) {
    return covariance_blocks(p, "pgo_covariance", false, q, t, sw, N, S, n_pairs, block_a, block_b, cov);
}

int pgo_get_jacobian_blocks(pgo_problem* p, int32_t kind, int64_t first, int64_t count, double* J1, double* J2, double* dr_ds) {
    if (!p || kind < 0 || kind > 2 || first < 0 || count < 0) return PGO_ERR_INVALID_ARG;
    if (p->graph_dirty) { p->err = "no linearisation available"; return PGO_ERR_STATE; }
    const int64_t E = kind == 0 ? p->G.rel.E : kind == 1 ? p->G.sw.E : p->G.n_prior;
    if (first + count > E) return PGO_ERR_INVALID_ARG;
    if (count == 0) return PGO_OK;
    int rc;
    if ((rc = set_device(p)) != PGO_OK) return rc;
    HIPCHK(p, p->d_tmp.ensure((size_t)count * 79));
    double* d1 = p->d_tmp.p; double* d2 = d1 + count * 36; double* ds = d2 + count * 36;
    launch_unpack_k1(p->G, kind, first, count, nullptr, d1, kind == 2 ? nullptr : d2, kind == 1 ? ds : nullptr, p->st);
    if (J1) HIPCHK(p, hipMemcpyAsync(J1, d1, count * 36 * sizeof(double), hipMemcpyDeviceToHost, p->st));
    if (J2 && kind != 2) HIPCHK(p, hipMemcpyAsync(J2, d2, count * 36 * sizeof(double), hipMemcpyDeviceToHost, p->st));
    if (dr_ds && kind == 1) HIPCHK(p, hipMemcpyAsync(dr_ds, ds, count * 7 * sizeof(double), hipMemcpyDeviceToHost, p->st));
    HIPCHK(p, hipStreamSynchronize(p->st));
    return PGO_OK;
}

int pgo_get_normal_blocks(pgo_problem* p, double* diag, double* grad, double* offdiag, double* sw_c, double* sw_hss, double* sw_gs) {
    if (!p) return PGO_ERR_INVALID_ARG;
    if (p->graph_dirty) { p->err = "no linearisation available"; return PGO_ERR_STATE; }
    int rc;
    if ((rc = set_device(p)) != PGO_OK) return rc;
    const int64_t Er = p->G.rel.E, Es = p->G.sw.E;
    if (diag && (rc = nodes_to_global(p, p->L.Hd, 36, diag)) != PGO_OK) return rc;
    if (grad && (rc = nodes_to_global(p, p->L.g, 6, grad)) != PGO_OK) return rc;
    if (offdiag && p->built_mf) {   // the matrix-free solver never forms J1^T J2: compute it for the parity hook only
        HIPCHK(p, p->d_Hoff.ensure((size_t)(p->G.rel.Epad + p->G.sw.Epad) * 36));
        p->L.Hoff = p->d_Hoff.p;
        launch_k2(p->G, p->L, true, p->st);
    }
    if (offdiag) {
        if (Er) HIPCHK(p, hipMemcpyAsync(offdiag, p->L.Hoff, Er * 36 * sizeof(double), hipMemcpyDeviceToHost, p->st));
        if (Es) HIPCHK(p, hipMemcpyAsync(offdiag + Er * 36, p->L.Hoff + (size_t)p->G.rel.Epad * 36, Es * 36 * sizeof(double), hipMemcpyDeviceToHost, p->st));
    }
    if (sw_c && Es) HIPCHK(p, hipMemcpyAsync(sw_c, p->L.c, Es * 12 * sizeof(double), hipMemcpyDeviceToHost, p->st));
    if (sw_hss && Es) HIPCHK(p, hipMemcpyAsync(sw_hss, p->L.hss, Es * sizeof(double), hipMemcpyDeviceToHost, p->st));
    if (sw_gs && Es) HIPCHK(p, hipMemcpyAsync(sw_gs, p->L.gs, Es * sizeof(double), hipMemcpyDeviceToHost, p->st));
    HIPCHK(p, hipStreamSynchronize(p->st));
    return PGO_OK;
}

int pgo_manifold_plus(pgo_problem* p, int64_t n, const double* quat, const double* t, const double* delta, double* quat_out, double* t_out) {
    if (!p || n < 0 || (n > 0 && (!quat || !delta || !quat_out))) return PGO_ERR_INVALID_ARG;
    if (n == 0) return PGO_OK;
    int rc;
    if ((rc = set_device(p)) != PGO_OK) return rc;
    const bool with_t = t != nullptr && t_out != nullptr;
    DBuf<double> d;
    HIPCHK(p, d.ensure((size_t)n * 20));
    double* dq = d.p; double* dd = dq + 4 * n; double* dqo = dd + 6 * n; double* dt = dqo + 4 * n; double* dto = dt + 3 * n;
    HIPCHK(p, hipMemcpyAsync(dq, quat, (size_t)n * 4 * sizeof(double), hipMemcpyHostToDevice, p->st));
    HIPCHK(p, hipMemcpyAsync(dd, delta, (size_t)n * 6 * sizeof(double), hipMemcpyHostToDevice, p->st));
    if (with_t) HIPCHK(p, hipMemcpyAsync(dt, t, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice, p->st));
    launch_manifold_plus(n, dq, with_t ? dt : nullptr, dd, dqo, with_t ? dto : nullptr, p->st);
    HIPCHK(p, hipMemcpyAsync(quat_out, dqo, (size_t)n * 4 * sizeof(double), hipMemcpyDeviceToHost, p->st));
    if (with_t) HIPCHK(p, hipMemcpyAsync(t_out, dto, (size_t)n * 3 * sizeof(double), hipMemcpyDeviceToHost, p->st));
    HIPCHK(p, hipStreamSynchronize(p->st));
    return PGO_OK;
}

int pgo_apply_normal_operator(pgo_problem* p, const double* x, double* y) {
    if (!p || !x || !y) return PGO_ERR_INVALID_ARG;
    if (!p->in_solve) { p->err = "pgo_apply_normal_operator needs an open solve (pgo_solve_begin)"; return PGO_ERR_STATE; }
    int rc;
    if ((rc = set_device(p)) != PGO_OK) return rc;
    bool ok = true;
    if ((rc = build_lm_system(p, &ok)) != PGO_OK) return rc;
    // x and y are arrays over ALL keyframes (multi-GPU: this rank applies its part to its keyframes, shared rows are summed)
    HIPCHK(p, p->d_io.ensure((size_t)p->N * 12));
    double* xin = p->d_io.p; double* yout = p->d_io.p + (size_t)p->N * 6;
    if ((rc = nodes_from_global(p, x, 6, xin)) != PGO_OK) return rc;
    if (p->built_mf) launch_mf_apply(p->G, p->F, p->ScMf, p->C, xin, yout, p->st);
    else launch_apply_operator(p->G, p->C, xin, yout, p->st);
    if ((rc = exchange_rows(p, yout, 6, nullptr, 0)) != PGO_OK) return rc;
    return nodes_to_global(p, yout, 6, y);
}

int pgo_device_synchronize(pgo_problem* p) {
    if (!p) return PGO_ERR_INVALID_ARG;
    int rc;
    if ((rc = set_device(p)) != PGO_OK) return rc;
    if ((rc = mg_fresh_install(p)) != PGO_OK) return rc;      // "everything this handle has in flight": the hierarchy worker of a fresh graph build too
    HIPCHK(p, hipStreamSynchronize(p->st));
    return PGO_OK;
}

const char* pgo_strerror(int code) {
    switch (code) {
        case PGO_OK: return "ok";
        case PGO_ERR_INVALID_ARG: return "invalid argument";
        case PGO_ERR_NO_DEVICE: return "no usable HIP device (libpgo has no CPU fallback)";
        case PGO_ERR_HIP: return "HIP runtime error";
        case PGO_ERR_OUT_OF_MEMORY: return "out of device memory";
        case PGO_ERR_STATE: return "call order violated";
        case PGO_ERR_COMM: return "RCCL error";
        case PGO_ERR_NUMERIC: return "non-finite value";
        default: return "unknown error";
    }
}
const char* pgo_last_error(const pgo_problem* p) { return p ? p->err.c_str() : ""; }
#ifndef PGO_SOURCE_SHA256
#define PGO_SOURCE_SHA256 "unknown (not built by _build.py)"
#endif
const char* pgo_build_info(void) { return "libpgo sources sha256:" PGO_SOURCE_SHA256; }

}  // extern "C"
