// pgo_pcg.hip — the linear solve of each LM system: the two-level preconditioner (aggregates, coarse operator, the comparison against plain block-Jacobi and its
// back-off across solves), the preconditioner choice of each system (build_system), and the PCG driver (iteration forms, chunking and capture, polling, the end game, the
// in-flight switch to the multigrid, the breakdown retry).  The LM controller around it is pgo_solver.hip.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pgo_handle.hpp"

namespace pgo {

// The two-level method's aggregates (consecutive keyframes) and the contribution lists of its dense coarse operator, for the graph as built: what a graph WITHOUT a multigrid
// hierarchy preconditions with.  Called by build_graph, and by mg_fresh_install when the hierarchy a worker thread prepared turns out not to coarsen (the synchronous path —
// several ranks — decides that inside build_graph; one GPU only learns it where the hierarchy is first needed: both end up with the same preconditioner).
int build_two_level_aggregates(pgo_problem* p) {
    CoarseState& c = p->coarse;
    const int64_t N = p->N, Er = p->rel.size(), Es = p->swe.size();
    const int32_t* g2l = p->local_ids ? p->g2l.data() : nullptr;
    auto L = [g2l](int32_t g) -> int32_t { return g2l ? g2l[g] : g; };
    int n_agg = p->opt.coarse_aggregates;
    // a graph with no more keyframes than `half` (256 by default) gets one aggregate per keyframe: the coarse operator IS the reduced system and the "preconditioner"
    // its dense inverse (a direct solve; the PCG around it only refines); larger graphs: at least 8 keyframes per aggregate, but not fewer than `half` aggregates — the
    // dense inverse (cubic in the aggregates) is what small graphs pay for (scripts/gpu_small_graphs.py) — and at most coarse_aggregates (768: measured on
    // chain-like session graphs of 6 000 - 23 000 keyframes, scripts/gpu_session_aggregates.py: 768 beats 512 by 3 - 45 %, 1024 and 1536 lose to the cubic inverse)
    const int half = std::min(n_agg / 2, 256);
    if (N <= half) n_agg = (int)N;
    else n_agg = (int)std::min<int64_t>(n_agg, std::max<int64_t>(N / 8, half));
    if (n_agg >= 2 && !p->local_ids && (N + n_agg - 1) / n_agg <= 1024) {    // aggregates of thousands of keyframes are never used (build_coarse)
        const int m = (int)((N + n_agg - 1) / n_agg);
        n_agg = (int)((N + m - 1) / m);
        std::vector<int32_t> agg_free((size_t)n_agg, 0);
        for (int64_t n = 0; n < N; ++n) if (p->h_node_free[n]) agg_free[n / m]++;
        // (block key, entry) pairs; key = a * n_agg + b with a <= b
        std::vector<std::pair<int64_t, int64_t>> ent;
        ent.reserve((size_t)N + 2 * (size_t)(Er + Es));
        for (int64_t n = 0; n < N; ++n) if (p->h_node_free[n]) ent.push_back({(int64_t)(n / m) * n_agg + n / m, (n << 3) | 0});
        auto edge = [&](int64_t e, int32_t c1, int32_t c2, int kind_fwd) {
            if (!p->h_node_free[c1] || !p->h_node_free[c2]) return;       // rows and columns of fixed keyframes are not part of the system
            const int64_t a = c1 / m, b = c2 / m;
            if (a < b) ent.push_back({a * n_agg + b, (e << 3) | kind_fwd});
            else if (a > b) ent.push_back({b * n_agg + a, (e << 3) | (kind_fwd + 1)});
            else { ent.push_back({a * n_agg + a, (e << 3) | kind_fwd}); ent.push_back({a * n_agg + a, (e << 3) | (kind_fwd + 1)}); }
        };
        for (int64_t e = 0; e < Er; ++e) edge(e, L(p->rel.c1[e]), L(p->rel.c2[e]), 1);
        for (int64_t e = 0; e < Es; ++e) edge(e, L(p->swe.c1[e]), L(p->swe.c2[e]), 3);
        for (int a = 0; a < n_agg; ++a) if (agg_free[a] == 0) ent.push_back({(int64_t)a * n_agg + a, -1});   // identity block: listed, no contribution
        std::stable_sort(ent.begin(), ent.end(), [](const std::pair<int64_t, int64_t>& x, const std::pair<int64_t, int64_t>& y) { return x.first < y.first; });
        std::vector<int64_t> blk_ptr, contrib;
        std::vector<int32_t> blk_ab;
        int64_t prev = -1;
        for (const auto& kv : ent) {
            if (kv.first != prev) { blk_ptr.push_back((int64_t)contrib.size()); blk_ab.push_back((int32_t)(kv.first / n_agg)); blk_ab.push_back((int32_t)(kv.first % n_agg)); prev = kv.first; }
            if (kv.second >= 0) contrib.push_back(kv.second);
        }
        blk_ptr.push_back((int64_t)contrib.size());
        const int n_blk = (int)blk_ab.size() / 2;
        const int nc = (6 * n_agg + 63) / 64 * 64;      // padded with a decoupled identity block (the dense kernels work on 64-wide tiles)
        HIPCHK(p, c.d_ccen.ensure((size_t)n_agg * 3)); HIPCHK(p, c.d_cd.ensure((size_t)N * 3)); HIPCHK(p, c.d_cAc.ensure((size_t)nc * nc)); HIPCHK(p, c.d_cAcf.ensure((size_t)nc * nc));
        HIPCHK(p, c.d_crc.ensure((size_t)nc * 2)); HIPCHK(p, c.d_cscr.ensure((size_t)nc * 64 + 4096)); HIPCHK(p, hipMemsetAsync(c.d_crc.p, 0, (size_t)nc * 2 * sizeof(double), p->st)); HIPCHK(p, c.d_cinfo.ensure(4));
        HIPCHK(p, c.d_cblk_ptr.upload(blk_ptr, p->st)); HIPCHK(p, c.d_ccontrib.upload(contrib, p->st)); HIPCHK(p, c.d_cblk_ab.upload(blk_ab, p->st)); HIPCHK(p, c.d_cagg_free.upload(agg_free, p->st));
        HIPCHK(p, hipStreamSynchronize(p->st));
        c.K = CoarseDev{n_agg, nc, m, n_blk, c.d_ccen.p, c.d_cd.p, c.d_cAc.p, c.d_crc.p, c.d_crc.p + nc, c.d_cblk_ptr.p, c.d_cblk_ab.p, c.d_ccontrib.p, c.d_cagg_free.p, c.d_cAcf.p};
        c.built = true;
    }
    return PGO_OK;
}

// Coarse operator of the two-level preconditioner for the system just built: Ac = P^T A P (deterministic assembly) and its dense inverse
// (blocked Gauss-Jordan kernels).  A coarse operator that is not numerically positive definite leaves the coarse space off for this iteration.
// force (pgo_apply_preconditioner): built whatever the solve's own comparison and the radius rule say, and without touching their state.
int build_coarse(pgo_problem* p, bool force) {
    CoarseState& c = p->coarse;
    c.active = false;
    const double t_coarse0 = now_s();
    // Where it pays: always when the aggregates are small (the coarse space is then a sizeable fraction of the problem: graphs up to
    // ~64 x coarse_aggregates keyframes), otherwise only at large trust regions, where the slow modes are the long wavelengths
    // (measured: scripts/gpu_coarse_ab.py).
    if (!c.built || p->opt.coarse_aggregates <= 0) return PGO_OK;
    if (!force && c.hist.mode == 2) {
        // dropped at a smaller trust region: the long wavelengths it removes dominate more and more as the radius grows, so it gets another
        // comparison once the radius is 9x (two accepted steps) beyond the one it lost at — at most twice per solve
        if (c.hist.retests >= 2 || c.hist.skip_all || !(p->lm.radius >= 9.0 * c.hist.drop_radius)) return PGO_OK;   // (eligibility by aggregate size / coarse_min_radius is checked below)
        ++c.hist.retests; c.hist.mode = 0;
    }
    if (!force && !(c.K.m <= 64 || (p->lm.radius >= p->opt.coarse_min_radius && c.K.m <= 1024))) return PGO_OK;   // aggregates of thousands of keyframes are too coarse to help
    if (c.geometry_epoch != p->lin_epoch) {          // the aggregates' centroids follow the poses of the current linearisation
        launch_coarse_geometry(p->G, c.K, p->d_pose[p->cur].p, p->st);
        c.geometry_epoch = p->lin_epoch;
    }
    launch_coarse_assemble(p->G, p->L, p->Sc, p->C, c.K, p->st);
    int32_t* fail = c.d_cinfo.p;
    HIPCHK(p, hipMemsetAsync(fail, 0, sizeof(int32_t), p->st));
    launch_coarse_invert(c.K, c.d_cscr.p, fail, p->st);
    if (debug_break_coarse()) launch_coarse_negate(c.K, p->st);
    int32_t h = 1;
    HIPCHK(p, hipMemcpyAsync(&h, fail, sizeof(h), hipMemcpyDeviceToHost, p->st));
    HIPCHK(p, hipStreamSynchronize(p->st));
    c.active = h == 0;
    if (p->opt.verbosity > 1) std::fprintf(stderr, "[pgo] coarse operator assembled and inverted in %.3f ms (since the start of build_coarse)\n", (now_s() - t_coarse0) * 1e3);
    if (p->opt.verbosity > 0) std::fprintf(stderr, "[pgo] coarse space: %d aggregates of %d keyframes, %d blocks, radius %.1e: %s\n", c.K.n_agg, c.K.m, c.K.n_blk, p->lm.radius, h == 0 ? "on" : "coarse operator not positive definite -> off");
    return PGO_OK;
}
// The back-off across solves.  At a solve's start: a handle in back-off skips the two-level method; one that kept it in the last solves uses it without the comparison.
void two_level_solve_begin(pgo_problem* p) {
    CoarseState& c = p->coarse;
    c.hist.retests = 0; c.hist.drop_radius = 0.0;
    if (c.hist.skip > 0) { c.hist.mode = 2; c.hist.skip_all = true; --c.hist.skip; }
    else { c.hist.mode = (c.hist.keep_streak % 4 != 0) ? 1 : 0; c.hist.skip_all = false; }
}
// At its end — (a solve that kept it: the next three solves of this handle use it without the comparison)
// a solve in which the coarse space lost every comparison: the following solves of this handle (incremental triggers on the same kind
// of graph) skip it, 1, 3, 7, 15 solves at a time, before comparing again; one win resets the back-off
void two_level_solve_end(pgo_problem* p) {
    CoarseState& c = p->coarse;
    if (c.hist.mode == 2 && !c.hist.skip_all) { c.hist.backoff = std::min(2 * c.hist.backoff + 1, 15); c.hist.skip = c.hist.backoff; }
    if (c.hist.mode == 1) ++c.hist.keep_streak; else if (c.hist.mode == 2 && !c.hist.skip_all) c.hist.keep_streak = 0;
}

static int build_system(pgo_problem* p, bool* ok) {
    PcgState& s = p->pcg;
    int rc;
    HIPCHK(p, hipMemsetAsync(p->d_flags.p + 4, 0, sizeof(int32_t), p->st));
    launch_build_rows(p->G, p->L, p->Sc, p->C, p->lm.radius, 1 /*one GPU: this handle adds Hd, g and the damping; multi-GPU: the keyframe's owner (G.own)*/, p->built_mf ? p->d_lam.p : nullptr, p->ScMf.a_inv, p->st);
    if ((rc = exchange_rows(p, p->C.Dtot, 36, p->C.b, 6)) != PGO_OK) return rc;   // reduced diagonal + rhs of shared keyframes
    launch_invert_rows(p->G, p->C, p->d_flags.p + 4, p->st);
    int32_t fail = 0;
    HIPCHK(p, hipMemcpyAsync(&fail, p->d_flags.p + 4, sizeof(int32_t), hipMemcpyDeviceToHost, p->st));
    HIPCHK(p, hipStreamSynchronize(p->st));
    if (p->local_ids) {      // a block that fails on one rank makes the step invalid on all of them (the ranks must take the same branch: collectives follow)
        std::vector<double> f(1, fail ? 1.0 : 0.0);
        if ((rc = host_allreduce(p, f, 2)) != PGO_OK) return rc;
        fail = f[0] != 0.0;
    }
    *ok = fail == 0;
    p->mg.active = false; s.mg_failed = false; p->C.extra_rz = 0; s.mg_start_deferred = false;
    // block-Jacobi-equivalent iterations this system is expected to need: those of the last fully solved system of this solve x sqrt(radius ratio); 0 = no prediction
    s.cg_predicted = (s.cg_prev_radius > 0.0 && p->lm.radius > 0.0) ? s.cg_prev_equiv * std::sqrt(p->lm.radius / s.cg_prev_radius) : 0.0;
    if (dense_mode(p)) { s.cg_predicted = 0.0; p->coarse.active = false; return PGO_OK; }      // the exact dense solver: no preconditioner to decide on
    if (*ok && p->mg.built) {
        // Which preconditioner the PCG of this LM system starts with.  Block-Jacobi iterations grow like sqrt(radius) from one accepted step
        // to the next, so the previous step of this solve predicts this one (a multigrid iteration counts as 4 block-Jacobi ones: it costs
        // ~2.5x and saves 4x or more on hard systems):  predicted >= 1.75 x mg_switch_iterations -> multigrid (from the first iteration, or after the prelude below);
        // predicted easier than that -> block-Jacobi, and the in-flight switch of run_pcg waits for twice the prediction (switching 400
        // iterations into a system that needs 520 throws the work away); no prediction (first step, after a rejected one) -> block-Jacobi with
        // the switch at mg_switch_iterations.  Depends on this solve's own history only.
        const double predicted = s.cg_predicted;
        // (round 3, with the smoothed cycle: start factors 1.0 - 2.25, waiting factors 1.5 - 2.0 and switch points 200 - 600 all within +-2 % on C3 and C4)
        // (with the deferred start and the regroup off the critical path, session 2 of round 3: start 1.0 - 2.25 x wait 1.5 / 2.0 on C3 0.311 - 0.333 s, C4 1.498 - 1.542 s; 1.75 / 2.0 is the best pair on both)
        const double start_factor = 1.75, wait_factor = 2.0;
        s.mg_switch_at = p->opt.mg_switch_iterations;
        if (predicted > 0.0 && predicted < start_factor * (double)p->opt.mg_switch_iterations) s.mg_switch_at = std::max(p->opt.mg_switch_iterations, (int)(wait_factor * predicted));
        // A system predicted hard gets the multigrid from the first iteration — unless the step can still be rejected early: most steps that ARE rejected follow a long
        // accepted one at a large radius, i.e. exactly the systems predicted hard, and block-Jacobi reaches the first pause (cg_early_tolerance, a few dozen iterations)
        // for a fraction of what the operators cost (C3, step 4: 32 ms for a step thrown away at 21 iterations).  Then the build waits for the pause (lm_step).
        const bool hard = p->opt.mg_switch_iterations <= 0 || predicted >= start_factor * (double)p->opt.mg_switch_iterations;
        // ... and only where a rejection is in the air (rejection_likely, pgo_lm.hpp): elsewhere — the accepted hard steps of C3 and C4 follow rho >= 0.89 — a prelude is
        // 74 block-Jacobi iterations the multigrid would not have needed: 3 ms x 5 on C3, 5 ms x 12 on C4
        s.mg_start_deferred = hard && rejection_likely(p->lm) && p->opt.mg_switch_iterations > 0 && p->opt.cg_early_tolerance > p->opt.cg_rel_tolerance;
        if (s.mg_start_deferred) {      // ... but not for long: a step that has not reached the pause within the prelude is a hard one that stays (late C3 systems need ~300 block-Jacobi iterations to 1e-2)
            const int prelude = 72;      // three chunks (measured on C3 / C4, 20 steps: 48 -> 0.392 / 1.500 s — C3's rejected step 4 needs 53 —, 72 -> 0.322 / 1.515 s, 96 -> 0.324 / 1.524 s)
            s.mg_switch_at = std::min(s.mg_switch_at, prelude);
        }
        if (hard && !s.mg_start_deferred && (rc = build_mg(p)) != PGO_OK) return rc;
    }
    else if (*ok && (rc = build_coarse(p)) != PGO_OK) return rc;
    return PGO_OK;
}
// The LM system at the current radius: the damping diagonal (a rejected or an invalid step keeps the one it had: reuse_diagonal), then the system and its preconditioner
int build_lm_system(pgo_problem* p, bool* ok) {
    if (!p->lm.reuse_diagonal) launch_lm_diag(p->G, p->L, p->Sc, p->opt.min_lm_diagonal, p->opt.max_lm_diagonal, p->st);
    return build_system(p, ok);
}
// One GPU, matrix-free matvec, tolerance not below 1e-11: the PCG runs in its single-reduction (Chronopoulos-Gear) form — matvec w = A u with the partials of u.w, then ONE
// vector kernel whose head re-reduces u.w and r.u together (pgo_kernels.hip: sr_head).  Decided by the options alone, so every phase of a paused PCG runs the same form.
// The two-level method: its FUSED three-kernel iteration has a single-reduction form of its own (launch_mf_apply_dot_live_coarse + launch_cg_update_restrict_sr) and runs it under the
// same gates (tolerance >= 1e-11, <= 150 000 keyframes); only its unfused form — aggregates too large for the update kernel's groups — stays classic.
bool single_reduction(const pgo_problem* p) {
    const bool two_level = p->coarse.active && !p->mg.active;
    // ... and only where the iteration is latency-bound: the form trades one partial-sum head (~4.5 us) for 96 more bytes per keyframe and iteration, which costs more than the
    // head from ~130 000 keyframes on — measured +1.4 % on C3 (100k) and +2...+7 % on 12k-60k-keyframe graphs, but -1.2 % on C4 (200k) and -1.7 % on C5 (1M)
    // (profiles/r05_single_reduction_graph_types.txt, r05_option_ab_c4_c5.txt)
    constexpr int64_t SINGLE_REDUCTION_MAX_KEYFRAMES = 150000;
    return p->opt.cg_single_reduction != 0 && !p->local_ids && p->built_mf && p->opt.cg_rel_tolerance >= 1e-11 && p->N_global <= SINGLE_REDUCTION_MAX_KEYFRAMES &&
           (!two_level || coarse_group_keyframes(p->coarse.K) > 0);
}
// The split update (pgo_internal.hpp: UpdRiderDev): which two launches of the cycle carry its riders — the two eligible launches with the fewest workgroups of their own (most of
// the GPU idle while they run), the earlier one the direction / solution half, the later one the block-Jacobi half.  A hierarchy with fewer than two eligible launches keeps
// the unsplit kernel.  A rule on the hierarchy alone: the same for eager launches, captured chunks and pgo_time_kernel.
static UpdSplit choose_split(const pgo_problem* p) {
    UpdSplit sp;
    if (debug_no_split_update() || mg_fine_view(p)) return sp;
    const MgCyclePlan P = mg_cycle_plan(p->mg.M, p->mg.levels, p->coarse.K, p->C.extra_rz, cg_grid_size(p->G), true, nullptr);
    uint32_t tiles[MgCyclePlan::CAPACITY];      // the eligible launches' own workgroups, by host ordinal
    int n = 0;
    for (int i = 0; i < P.n; ++i) if (P.steps[i].rider) tiles[n++] = P.steps[i].grid;
    if (n < 2) return sp;
    int a = 0;
    for (int e = 1; e < n; ++e) if (tiles[e] < tiles[a]) a = e;
    int b = a == 0 ? 1 : 0;
    for (int e = 0; e < n; ++e) if (e != a && tiles[e] < tiles[b]) b = e;
    sp.host_a = std::min(a, b); sp.host_b = std::max(a, b);
    int da, db;
    if (debug_split_hosts(&da, &db) && db < n) { sp.host_a = da; sp.host_b = db; }
    return sp;
}
PcgForm choose_form(const pgo_problem* p, bool this_rank_only) {
    PcgForm f{PcgForm::classic_csr, PcgForm::none, 0};
    const bool mg = p->mg.active, two_level = p->coarse.active && !mg;
    // two-level preconditioner in three kernels per iteration (prolongation inside the matvec, restriction inside the update, r.(P y) from the dense solve)
    const bool fused_coarse = !p->local_ids && two_level && p->built_mf && coarse_group_keyframes(p->coarse.K) > 0;
    if (p->local_ids && !this_rank_only) f.rec = PcgForm::ranks;
    else if (fused_coarse) f.rec = single_reduction(p) ? PcgForm::sr_coarse : PcgForm::classic_coarse;
    else if (single_reduction(p)) f.rec = PcgForm::sr;
    else if (p->built_mf) f.rec = PcgForm::classic_mf;
    if (fused_coarse) f.fused_parts = coarse_update_grid(p->G, p->coarse.K);
    else if (mg) f.post = f.rec != PcgForm::ranks && p->mg.M.blk_tab != nullptr ? PcgForm::mg_restricted : PcgForm::mg_cycle;      // (blk_tab: the vector update also restricts the new residual to level 1)
    else if (two_level) f.post = PcgForm::two_level;
    if (f.rec == PcgForm::sr && f.post == PcgForm::mg_restricted) f.split = choose_split(p);
    return f;
}
// w = A u (with the partials of u.w; the classic forms: the new direction first, and the convergence test against tol2; the fused two-level method: the prolongation inside)
void pcg_matvec(pgo_problem* p, const PcgForm& f, int k, double tol2) {
    if (f.rec == PcgForm::ranks && p->built_mf) launch_mf_apply_dot(p->G, p->F, p->ScMf, p->C, p->C.z, p->C.q, p->st);   // w = A_r u and the partials of u.w in one kernel
    else if (f.rec == PcgForm::ranks) { launch_apply_operator(p->G, p->C, p->C.z, p->C.q, p->st); launch_cgcg_dots(p->G, p->C, p->st); }
    else if (f.rec == PcgForm::sr) launch_mf_apply_dot_live(p->G, p->F, p->ScMf, p->C, p->st);      // (no head: it only asks whether the PCG has stopped)
    else if (f.rec == PcgForm::sr_coarse) launch_mf_apply_dot_live_coarse(p->G, p->F, p->ScMf, p->C, p->coarse.K, k > 0 ? 1 : 0, p->st);      // w = A (z_bj + P y) (iteration 0: the PCG start has left the complete u in C.z)
    else if (f.rec == PcgForm::classic_coarse) launch_mf_spmv_coarse(p->G, p->F, p->ScMf, p->C, p->coarse.K, k, tol2, f.fused_parts, k > 0 ? 1 : 0, p->st);
    else if (f.rec == PcgForm::classic_mf) launch_mf_spmv(p->G, p->F, p->ScMf, p->C, k, tol2, p->st);
    else launch_cg_spmv(p->G, p->C, k, tol2, p->st);
}
// the vector update (the single-reduction forms: with the iteration's one reduction point; `first`: also when a PCG that stopped before its first update is resumed — p = s = 0 still)
int pcg_update(pgo_problem* p, const PcgForm& f, int k) {
    const int first = k == 0 ? 1 : 0, n_pq = p->built_mf ? mf_grid_size(p->F) : cg_grid_size(p->G);
    const bool restricted = f.post == PcgForm::mg_restricted;
    const MgState& m = p->mg;
    if (f.rec == PcgForm::ranks) {
        // The iteration's exchanges: the partial rows of w of the keyframes this rank shares go to the ranks sharing them (one group of sends / receives), the parts are
        // summed in ascending rank order; [delta, gamma] by ONE all-reduce of two doubles.  Then the update.
        int rc;
        launch_cg_reduce2_live(p->C, p->C.part_pq, n_pq, p->C.part_rz, cg_grid_size(p->G), p->d_xscal.p, p->st);
        if ((rc = exchange_rows(p, p->C.q, 6, nullptr, 0, p->C.flags)) != PGO_OK || (rc = allreduce(p, p->d_xscal.p, 2, 0)) != PGO_OK) return rc;
        launch_cgcg_update(p->G, p->C, k, first, p->st, nullptr, nullptr, p->d_xscal.p);
        ++p->st_pcg_iterations;
    } else if (f.rec == PcgForm::sr_coarse) launch_cg_update_restrict_sr(p->G, p->C, p->coarse.K, k, first, k > 0 ? 1 : 0, n_pq, p->st);
    else if (f.rec == PcgForm::classic_coarse) launch_cg_update_restrict(p->G, p->C, p->coarse.K, k, n_pq, p->st);
    else if (f.rec == PcgForm::sr && restricted && f.split.on()) launch_cg_update_mg_crit(p->G, p->C, m.M, m.levels, p->coarse.K, k, first, n_pq, p->st);      // (pcg_precond's cycle carries the rest)
    else if (f.rec == PcgForm::sr && restricted) launch_cg_update_mg_sr(p->G, p->C, m.M, m.levels, p->coarse.K, k, first, n_pq, p->st);
    else if (f.rec == PcgForm::sr) launch_cg_update_sr(p->G, p->C, k, first, n_pq, p->st);
    else if (restricted) launch_cg_update_mg(p->G, p->C, m.M, m.levels, p->coarse.K, k, n_pq, p->st);
    else launch_cg_update(p->G, p->C, k, n_pq, p->st);
    return PGO_OK;
}
// u = M^-1 r beyond block-Jacobi.  The classic forms leave the new residual in the OTHER r buffer, its r.z partials go to the other parity's slots.
int pcg_precond(pgo_problem* p, const PcgForm& f, int k) {
    double* const part_rz = p->C.part_rz + (size_t)((k & 1) ^ 1) * RZ_STRIDE;
    const double* const r = f.single_red() || (k & 1) ? p->C.r : p->C.r2;
    if (f.fused_coarse()) launch_coarse_solve_dot(p->coarse.K, p->C.flags, part_rz + f.fused_parts, p->st);      // the dense solve: y and the coarse part of r.u
    else if (f.mg() && f.rec == PcgForm::ranks) return mg_apply_ranks(p, true);      // u = D^-1 r + P0 V(P0^T r)
    else if (f.mg()) {
        MgCycleArgs a;
        a.r = r; a.part_rz = part_rz; a.inside_iteration = true; a.restricted = f.post == PcgForm::mg_restricted;
        if (f.rec == PcgForm::sr && a.restricted && f.split.on()) { a.split = &f.split; a.parity = k & 1; a.first = k == 0 ? 1 : 0; }      // (hosts chosen on the plan this cycle walks: choose_split)
        return mg_cycle(p, p->C, a);
    }
    else if (f.post == PcgForm::two_level) launch_coarse_apply(p->G, p->C, p->coarse.K, r, p->C.z, part_rz, true, p->st);
    return PGO_OK;
}
// The PCG start: r = b (- A x with a warm start: q = A x first), z = M^-1 r, the scalars of iteration 0.
// One GPU with the two-level method or the multigrid: z = D^-1 r + P Ac^-1 P^T r (or the cycle): the coarse term is added to z and to the r.z partials before the scalars are formed.
// Several ranks: u = M^-1 r, p = s = 0; part_rz <- owner-weighted partials of gamma_0 (summed over ranks with the first iteration's scalars), part_pq <- partials of b.D^-1 b,
// summed over ranks here once: the reference norm of the stopping test.  With the multigrid: the distributed cycle (mg_apply_ranks).
int pcg_start(pgo_problem* p, const PcgForm& f, bool warm, double tol2) {
    int rc;
    if (warm) {
        if (p->built_mf) launch_mf_apply(p->G, p->F, p->ScMf, p->C, p->C.x, p->C.q, p->st);
        else launch_apply_operator(p->G, p->C, p->C.x, p->C.q, p->st);
        if ((rc = exchange_rows(p, p->C.q, 6, nullptr, 0)) != PGO_OK) return rc;
    }
    if (f.rec == PcgForm::ranks) {
        const int g = launch_cg_init_vectors(p->G, p->C, warm ? 1 : 0, p->st);
        if (f.mg() && (rc = mg_apply_ranks(p, false)) != PGO_OK) return rc;      // z += P0 V(P0^T r): the restriction covers the rank's own aggregates (all their keyframes are local)
        double* bb = p->C.scal + 12;
        launch_reduce(p->C.part_pq, g, 0, bb, p->st);
        if ((rc = allreduce(p, bb, 1, 0)) != PGO_OK) return rc;
        launch_cgcg_scalars_init(p->C, bb, tol2, p->st);
    } else if (f.precond() == 0) {
        launch_cg_init(p->G, p->C, warm ? 1 : 0, tol2, p->st);
    } else {
        int g = launch_cg_init_vectors(p->G, p->C, warm ? 1 : 0, p->st);
        const int g_bb = g;      // the slots of part_pq that hold the partials of b.D^-1 b
        if (f.mg()) mg_cycle(p, p->C, MgCycleArgs{});
        else launch_coarse_apply(p->G, p->C, p->coarse.K, p->C.r, p->C.z, p->C.part_rz, false, p->st);
        if (f.fused_coarse()) {    // z is complete here: the slots the fused kernels will use beyond the start-up kernels' stay zero for this parity
            HIPCHK(p, hipMemsetAsync(p->C.part_rz + g, 0, (size_t)(f.fused_parts + p->C.extra_rz - g) * sizeof(double), p->st));
            g = f.fused_parts;
        }
        launch_cg_init_scalars(p->C, g, g_bb, tol2, p->st);
    }
    return PGO_OK;
}
int pcg_iteration(pgo_problem* p, const PcgForm& f, int k, double tol2) {
    int rc;
    pcg_matvec(p, f, k, tol2);
    if ((rc = pcg_update(p, f, k)) != PGO_OK) return rc;
    return pcg_precond(p, f, k);
}

namespace {

// iterations per chunk: even, so that the r/p ping-pong parity repeats from chunk to chunk
int chunk_length(const pgo_problem* p, const PcgForm& f) {
    int e = std::max(2, p->opt.cg_check_every) & ~1;
    // captured chunks stay at <= 72 kernel nodes (rocprofv3 7.2 crashes while a graph of 120 nodes is captured under --kernel-trace; 80 are fine): five kernels
    // per iteration with the coarse space in its unfused form -> 12 iterations, three in the fused form -> 24
    if (f.precond() == 1) e = std::min(e, f.fused_coarse() ? 24 : 12);
    if (!f.mg()) return e;
    const MgState& m = p->mg;
    int n_sm = 0;
    for (int l = 0; l < m.M.n_levels; ++l) n_sm += (m.levels[l].smoothed && !m.levels[l].rt_valf) ? 1 : 0;      // two more kernels per cycle for every level whose smoothed prolongator is applied implicitly (none with the explicit transfer operator)
    if (f.rec == PcgForm::ranks) return std::min(e, std::max(2, (72 / (6 * m.M.n_levels + 12)) & ~1));      // (every exchange is a pack kernel, the transfer and an unpack kernel)
    return std::max(2, (72 / (2 * m.M.n_levels + 3 + 2 * n_sm)) & ~1);   // at most 2 n_levels + 1 cycle kernels + matvec + update per iteration (one less with the restriction inside the update)
}
// END GAME (round 5, one GPU).  A chunk enqueued past convergence is a string of early-exit kernels (~2 us each: 100-150 us per stopped PCG with a chunk in flight, more
// than a tenth of a session-sized PCG).  The polled r.z values give the convergence rate; once the predicted remaining iterations fall below two chunks the host stops
// running ahead: it enqueues what the prediction asks for (+15 % + 4 iterations: an early-exit iteration costs a quarter of a host round trip), eagerly, and polls at once.
// Chunk lengths depend on the device's own r.z values alone — the PCG's iterates do not depend on how its iterations are cut into chunks.
struct EndGame {
    bool on = false, tight = false, have = false; int next = 0, k0 = 0; double rz0 = 0.0;
    void snapshot(pgo_problem* p) { if (on) launch_cg_poll(p->C, p->pcg.poll[2].flags, p->pcg.poll[2].scal, p->st); have = false; }      // (read only after a later poll's event: stream order)
    void update(const pgo_problem* p, int slot, int k, int every, double tol2) {      // a completed poll: new rate estimate from the last two points, length of the next chunk
        if (!on) return;
        const PcgState::Poll* poll = p->pcg.poll;
        const int kk = poll[slot].flags[2]; const double rz = poll[slot].scal[1], bb = poll[slot].scal[0];
        if (!have) { k0 = poll[2].flags[2]; rz0 = poll[2].scal[1]; have = true; }
        tight = false; next = every;
        if (rz > 0.0 && bb > 0.0 && rz0 > 0.0 && kk > k0 && rz < rz0) {
            const double lr = std::log(rz / rz0) / (double)(kk - k0);
            const double need = std::log(tol2 * bb / rz);
            const double left = need < 0.0 ? need / lr - (double)(k - kk) : 0.0;      // iterations still to run beyond what is already enqueued
            if (left < 2.0 * (double)every) {
                tight = true;
                const int want = (int)std::ceil(std::max(left, 0.0) * 1.15 + 4.0);
                next = std::max(2, std::min(every, (want + 1) & ~1));
            }
        }
        if (kk > k0) { k0 = kk; rz0 = rz; }
    }
};
// what one PCG phase carries from chunk to chunk
struct PcgRun {
    PcgForm f; double tol2; int cap; bool want_graph; int every = 2, k = 0, n_chunks = 0, waited = -1; EndGame eg;
    int ex_k0 = -1; double ex_rz0 = 0.0;      // first polled (iteration, r.z) of this phase: base of the in-flight switch's convergence-rate estimate
};
// hipGraph: capture one chunk (iterations 2 .. 2+every-1: no `first` kernel, even start) once per graph build and preconditioner, and replay it
void ensure_graph(pgo_problem* p, const PcgRun& R, bool may_capture) {
    PcgState& s = p->pcg;
    PcgState::CapturedChunk& cc = s.cg_chunk[R.f.precond()];
    const bool sr = R.f.single_red();
    if (!R.want_graph || s.cg_graph_failed || (cc.exec != nullptr && cc.epoch == s.build_epoch && cc.len == R.every && cc.scale == mg_scale(p) && cc.sr == sr)) { s.cg_graph = R.want_graph && !s.cg_graph_failed ? cc.exec : nullptr; return; }
    if (!may_capture) { s.cg_graph = nullptr; return; }
    if (cc.exec) { (void)hipGraphExecDestroy(cc.exec); cc.exec = nullptr; }
    hipGraph_t gr = nullptr;
    bool ok = hipStreamBeginCapture(p->st, hipStreamCaptureModeThreadLocal) == hipSuccess;
    if (ok) {
        for (int j = 0; j < R.every; ++j) (void)pcg_iteration(p, R.f, 2 + j, R.tol2);
        ok = hipStreamEndCapture(p->st, &gr) == hipSuccess && gr != nullptr;
    }
    const double t_inst = now_s();
    if (ok) ok = hipGraphInstantiate(&cc.exec, gr, nullptr, nullptr, 0) == hipSuccess;
    if (p->opt.verbosity > 1) std::fprintf(stderr, "[pgo] PCG chunk of %d iterations (preconditioner %d) captured, instantiated in %.2f ms\n", R.every, R.f.precond(), (now_s() - t_inst) * 1e3);
    if (gr) (void)hipGraphDestroy(gr);
    if (!ok) { cc.exec = nullptr; s.cg_graph_failed = true; (void)hipGetLastError(); }
    else { cc.epoch = s.build_epoch; cc.len = R.every; cc.scale = mg_scale(p); cc.sr = sr; }
    s.cg_graph = cc.exec;
}
int enqueue_poll(pgo_problem* p, int slot) {
    PcgState& s = p->pcg;
#ifdef PGO_POLL_BY_COPY
    HIPCHK(p, hipMemcpyAsync(s.poll[slot].flags, p->C.flags, 3 * sizeof(int32_t), hipMemcpyDeviceToHost, p->st));
    HIPCHK(p, hipMemcpyAsync(s.poll[slot].scal, p->C.scal, 3 * sizeof(double), hipMemcpyDeviceToHost, p->st));
#else
    launch_cg_poll(p->C, s.poll[slot].flags, s.poll[slot].scal, p->st);
#endif
    HIPCHK(p, hipEventRecord(s.poll_ev[slot], p->st));
    return PGO_OK;
}
bool may_switch_to_mg(const pgo_problem* p) { return p->mg.built && !p->mg.active && !p->pcg.mg_failed; }

// A system without a prediction (the first of a solve, the first after rejected steps) need not burn mg_switch_iterations block-Jacobi iterations to be
// recognised as hard: the polled r.z values give its convergence rate, and a system that would need >= the start threshold in total at that rate (and at
// least twice what it has done) switches now.  Depends on the solve's own data alone; several ranks: r.z and the reference norm are all-reduced values, every
// rank sees the same bits and takes the same branch.
void switch_estimate(pgo_problem* p, PcgRun& R, int slot) {
    const pgo_options& o = p->opt;
    PcgState& s = p->pcg;
    if (!may_switch_to_mg(p) || s.mg_start_deferred || o.mg_switch_iterations <= 0 || R.k >= s.mg_switch_at) return;
    const int kk = s.poll[slot].flags[2]; const double rz = s.poll[slot].scal[1], bb = s.poll[slot].scal[0];
    if (!(rz > 0.0 && bb > 0.0)) return;
    if (R.ex_k0 < 0) { if (kk >= 24) { R.ex_k0 = kk; R.ex_rz0 = rz; } }
    else if (kk >= 96 && kk > R.ex_k0) {
        const double lr = std::log(rz / R.ex_rz0) / (double)(kk - R.ex_k0);                   // log reduction per iteration (negative while converging)
        const double need = std::log(o.cg_rel_tolerance * o.cg_rel_tolerance * bb / rz);      // what is left down to the final tolerance (negative)
        const double total = lr < 0.0 ? (double)kk + need / lr : 1e30;
        if (total >= 1.75 * (double)o.mg_switch_iterations && total >= 2.0 * (double)kk) s.mg_switch_at = std::min(s.mg_switch_at, R.k);
    }
}
// block-Jacobi -> multigrid inside one system: operators built now, PCG restarted from the current iterate (`so_far` iterations are booked as cg_extra)
int switch_to_mg(pgo_problem* p, PcgRun& R, int so_far) {
    int rc = build_mg(p);
    if (rc != PGO_OK) return rc;
    if (!p->mg.active) { p->pcg.mg_failed = true; return PGO_OK; }
    p->pcg.cg_extra += so_far;
    R.f = choose_form(p);
    if ((rc = pcg_start(p, R.f, true, R.tol2)) != PGO_OK) return rc;
    R.k = 0; R.n_chunks = 0; R.waited = -1; R.every = chunk_length(p, R.f);
    R.eg.tight = false; R.eg.next = R.every; R.eg.have = false; R.eg.snapshot(p);
    ensure_graph(p, R, true);      // a system that needed the switch is a long one
    return PGO_OK;
}

}  // namespace

int run_pcg(pgo_problem* p, CgResult* res, const PcgPhase& ph) {
    const pgo_options& o = p->opt;
    PcgState& s = p->pcg;
    PcgRun R{choose_form(p), ph.tol * ph.tol, ph.max_iterations > 0 ? ph.max_iterations : o.cg_max_iterations};
    const bool multi = R.f.rec == PcgForm::ranks;
    int rc;
    if (R.f.fused_coarse()) p->C.extra_rz = coarse_solve_grid(p->coarse.K);      // the update kernel's r.z partials take `fused_parts` slots, the solve's C.extra_rz slots behind them
    else if (!p->mg.active) p->C.extra_rz = 0;
    if (ph.resume >= 0) launch_cg_set_tolerance(p->C, R.tol2, p->st);
    else if ((rc = pcg_start(p, R.f, ph.warm, R.tol2)) != PGO_OK) return rc;      // (a warm start: after a rejected step the system keeps H and only the damping grows)
    R.k = ph.resume >= 0 ? ph.resume : 0;
    R.every = chunk_length(p, R.f);
    // Several ranks: only where the transport's collectives can be captured (pgo_comm.hip: RCCL, opt-in; not a caller-supplied collective, a host callback)
    R.want_graph = o.cg_use_graph && !s.cg_graph_failed && (!p->local_ids || (p->comm && p->comm->graph_capturable()));
    // Capture + instantiation cost about a millisecond: a PCG pays it only once it has run `graph_after` iterations eagerly (a graph that is rebuilt for every
    // solve — the reference's sessions: one new loop edge, one solve — and converges in a few hundred iterations never does; eager launches keep up with
    // 5-8 us kernels: measured 18.5 vs 19.4 ms at 300 keyframes, 64.0 vs 64.6 ms at 3000)
    const int graph_after = debug_graph_after();
    ensure_graph(p, R, R.k >= graph_after);
    // Chunks of `every` iterations; the convergence flag of chunk j is read (pinned memory + event) only AFTER chunk j+1 has been
    // enqueued, so the GPU never drains while the host polls.  A chunk enqueued after convergence is a string of early-exit kernels.
    bool done = false;
    R.eg.on = o.cg_end_game != 0 && !multi;
    // a system predicted hard whose step has survived the first early-rejection pause (lm_step): the multigrid takes over from the iterate the pause left
    if (ph.switch_now && ph.resume >= 0 && may_switch_to_mg(p) && (rc = switch_to_mg(p, R, ph.resume)) != PGO_OK) return rc;
    R.eg.next = R.every;
    if (ph.resume >= 0 || R.k == 0) R.eg.snapshot(p);
    while (R.k < R.cap && !done) {
        if (R.eg.tight && R.n_chunks > 0 && R.waited < R.n_chunks - 1) {      // end game: the chunk in flight is waited for before anything else is enqueued
            HIPCHK(p, hipEventSynchronize(s.poll_ev[(R.n_chunks - 1) & 1]));
            R.waited = R.n_chunks - 1;
            if (s.poll[R.waited & 1].flags[0]) { done = true; break; }
            R.eg.update(p, R.waited & 1, R.k, R.every, R.tol2);
        }
        // (a phase that only has to reach an early-rejection pause's loose tolerance is a matter of a few iterations: its first chunk is short, the rate estimate takes over from there)
        const int first_short = R.eg.on && R.n_chunks == 0 && ph.tol >= 5e-3 ? std::min(R.every, 8) : R.every;
        const int chunk = std::min(R.eg.tight ? R.eg.next : first_short, R.cap - R.k);
        if (R.want_graph && !s.cg_graph_failed && !s.cg_graph && R.k >= graph_after && (R.k & 1) == 0) ensure_graph(p, R, true);
        if (R.k >= 2 && chunk == R.every && R.want_graph && s.cg_graph && (R.k & 1) == 0) {
            HIPCHK(p, hipGraphLaunch(s.cg_graph, p->st));
            R.k += R.every;
        } else {
            // iterations 0,1 run eagerly (iteration 0 has its own kernel arguments); an odd resume index takes one eager iteration to realign
            const int n = R.k == 0 ? std::min(2, chunk) : ((R.k & 1) ? 1 : chunk);
            const bool startup = R.k == 0 || (R.k & 1);
            for (int j = 0; j < n; ++j, ++R.k) if ((rc = pcg_iteration(p, R.f, R.k, R.tol2)) != PGO_OK) return rc;
            if (startup && R.k < R.cap) continue;     // no host poll after the start-up iterations
        }
        if ((rc = enqueue_poll(p, R.n_chunks & 1)) != PGO_OK) return rc;
        // the first two chunks are polled immediately (short solves finish there); afterwards one chunk stays in flight
        const int check = (R.n_chunks < 2 || R.eg.tight) ? R.n_chunks : R.n_chunks - 1;
        if (check > R.waited) {
            HIPCHK(p, hipEventSynchronize(s.poll_ev[check & 1]));
            R.waited = check;
            if (s.poll[check & 1].flags[0]) done = true;
            else R.eg.update(p, check & 1, R.k, R.every, R.tol2);
            if (!done) switch_estimate(p, R, check & 1);
        }
        ++R.n_chunks;
        // Hybrid preconditioning: most LM systems (small trust regions, steps about to be rejected) are solved by block-Jacobi in a few
        // hundred cheap iterations; one that is not done after mg_switch_iterations is a hard one, and from there the multigrid (4x fewer
        // iterations or better at ~3x the price) takes over: operators built now, PCG restarted from the current iterate.
        if (!done && may_switch_to_mg(p) && R.k >= s.mg_switch_at && R.k < R.cap) {     // (several ranks: every quantity tested here is the same on all of them)
            int32_t hflags[3] = {0, 0, 0};
            HIPCHK(p, hipMemcpyAsync(hflags, p->C.flags, sizeof(hflags), hipMemcpyDeviceToHost, p->st));
            HIPCHK(p, hipStreamSynchronize(p->st));
            if (hflags[0]) { done = true; (void)enqueue_poll(p, R.n_chunks & 1); ++R.n_chunks; break; }
            if ((rc = switch_to_mg(p, R, hflags[2])) != PGO_OK) return rc;
        }
    }
    int32_t hflags[3] = {0, 0, 0}; double hscal[3] = {0, 0, 0};
    if (R.n_chunks > 0) {   // the state after the LAST enqueued chunk is the final one (kernels past convergence do nothing)
        HIPCHK(p, hipEventSynchronize(s.poll_ev[(R.n_chunks - 1) & 1]));
        std::memcpy(hflags, s.poll[(R.n_chunks - 1) & 1].flags, sizeof(hflags));
        std::memcpy(hscal, s.poll[(R.n_chunks - 1) & 1].scal, sizeof(hscal));
    } else {
        HIPCHK(p, hipMemcpyAsync(hflags, p->C.flags, sizeof(hflags), hipMemcpyDeviceToHost, p->st));
        HIPCHK(p, hipMemcpyAsync(hscal, p->C.scal, sizeof(hscal), hipMemcpyDeviceToHost, p->st));
        HIPCHK(p, hipStreamSynchronize(p->st));
    }
    res->converged = hflags[0] != 0 && hflags[1] == 0;
    if (!hflags[0] && !multi) {   // iteration cap reached: one more convergence test so that scal[1] holds the last r.z (x is already final)
        launch_cg_set_tolerance(p->C, 1e300, p->st);
        // the classic forms: the matvec's test; single-reduction: the whole iteration (its update's head finds r.u below the tolerance: scal[1] <- r.u, nothing else moves)
        if (!R.f.single_red()) pcg_matvec(p, R.f, R.k, 1e300);
        else if ((rc = pcg_iteration(p, R.f, R.k, 1e300)) != PGO_OK) return rc;
        HIPCHK(p, hipMemcpyAsync(hflags, p->C.flags, sizeof(hflags), hipMemcpyDeviceToHost, p->st));
        HIPCHK(p, hipMemcpyAsync(hscal, p->C.scal, sizeof(hscal), hipMemcpyDeviceToHost, p->st));
        HIPCHK(p, hipStreamSynchronize(p->st));
    }
    res->iterations = hflags[2];
    res->breakdown = hflags[1] != 0;
    res->rel_residual = hscal[0] > 0 ? std::sqrt(std::max(0.0, hscal[1]) / hscal[0]) : 0.0;
    return PGO_OK;
}

// What follows the PCG of an LM system (after lm_step's pauses; `evaluated`: the step was rejected at one): the comparison against plain block-Jacobi, the preconditioner
// used, the breakdown retry, and the block-Jacobi-equivalent work that predicts the next system (build_system).
int finish_system(pgo_problem* p, CgResult* cg, bool evaluated, int* precond_used) {
    const pgo_options& o = p->opt;
    CoarseState& c = p->coarse; PcgState& s = p->pcg;
    int rc;
    // The coarse space pays by a large factor or not at all (it can even cost iterations on chains that odometry weights cut into
    // many loose pieces), so once per solve — at the first full-accuracy step that used it — plain block-Jacobi gets the SAME
    // iteration budget on the same system: if it does not converge within it the coarse space stays for the rest of
    // the solve, otherwise it is dropped.  The test costs at most as many iterations as the coarse run took.
    if (c.active && c.hist.mode == 0 && !evaluated && !cg->breakdown && cg->converged) {
        HIPCHK(p, p->d_tmp.ensure((size_t)p->N * 6));
        HIPCHK(p, hipMemcpyAsync(p->d_tmp.p, p->C.x, (size_t)p->N * 6 * sizeof(double), hipMemcpyDeviceToDevice, p->st));
        c.active = false;
        CgResult plain{0, false, 0.0, false};
        // an iteration with the coarse space costs 2.6-2.8x a plain one (three more kernels at the latency floor, measured from 200 to
        // 20k keyframes): equal TIME budgets
        if ((rc = run_pcg(p, &plain, PcgPhase{o.cg_rel_tolerance, -1, false, false, std::max(3 * cg->iterations, 2 * (std::max(2, o.cg_check_every) & ~1))})) != PGO_OK) return rc;
        if (plain.converged && !plain.breakdown) {      // block-Jacobi alone is at least as fast here
            // lost although it needed clearly fewer iterations: worth another comparison at a larger radius; lost without even that
            // (the aggregates' rigid modes are not this graph's slow modes): no more comparisons in this solve
            if ((double)plain.iterations < 1.2 * (double)cg->iterations) c.hist.retests = 2;
            c.hist.mode = 2; cg->iterations += plain.iterations; c.hist.drop_radius = p->lm.radius;
        }
        else {
            c.hist.mode = 1; c.active = true; c.hist.backoff = 0;
            HIPCHK(p, hipMemcpyAsync(p->C.x, p->d_tmp.p, (size_t)p->N * 6 * sizeof(double), hipMemcpyDeviceToDevice, p->st));
            cg->iterations += plain.iterations;
        }
    }
    // A breakdown under the multigrid (its cycle was not positive definite on this system — a smoother at its stability limit) or under the two-level method (its
    // dense coarse inverse is applied rounded to fp32: at large trust-region radii the coarse operator's condition number exceeds what fp32 resolves, and the rounded
    // inverse need not be positive definite) is not the system's fault: the same system is solved again by plain block-Jacobi before the step may count as invalid.
    // Ceres' exact factorisation never turns a solvable step into an invalid one (reference src/PoseGraphSLAM.cpp:1903).
    *precond_used = p->mg.active ? PGO_PRECOND_MULTIGRID : (c.active ? PGO_PRECOND_TWO_LEVEL : PGO_PRECOND_BLOCK_JACOBI);
    if (cg->breakdown && (p->mg.active || c.active) && !evaluated) {
        if (o.verbosity > 0) std::fprintf(stderr, "[pgo] %s: PCG breakdown at radius %.1e after %d iterations (preconditioner not positive definite) -> block-Jacobi for this system\n",
                                          p->mg.active ? "multigrid" : "two-level method", p->lm.radius, cg->iterations);
        if (p->mg.active) { p->mg.active = false; s.mg_failed = true; }
        c.active = false;      // (this system only: build_coarse decides again for the next one)
        p->C.extra_rz = 0;
        s.cg_extra += cg->iterations;
        ++p->sum.pcg_retries;
        *precond_used = PGO_PRECOND_BLOCK_JACOBI | PGO_PRECOND_RETRIED;
        // The iterate the broken-down PCG stopped at is a valid starting point (x_k with r_k = b - A x_k; a breakdown leaves x untouched): warm start.  Should that one
        // break down as well (a NaN that reached x), the system is solved from zero.
        if ((rc = run_pcg(p, cg, PcgPhase{o.cg_rel_tolerance, -1, true})) != PGO_OK) return rc;
        if (cg->breakdown) { s.cg_extra += cg->iterations; if ((rc = run_pcg(p, cg, PcgPhase{o.cg_rel_tolerance})) != PGO_OK) return rc; }
    }
    // block-Jacobi-equivalent work of this system, for the next system's choice of preconditioner (build_system)
    if (!evaluated && !cg->breakdown) {
        const double equiv = p->mg.levels[0].smoothed ? 8.0 : 4.0;     // block-Jacobi iterations one multigrid iteration stands for on a hard system
        s.cg_prev_equiv = (double)s.cg_extra + (p->mg.active ? equiv : 1.0) * (double)cg->iterations; s.cg_prev_radius = p->lm.radius;
    }
    return PGO_OK;
}

}  // namespace pgo
