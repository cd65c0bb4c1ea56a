// pgo_solver.hip — host side of libpgo: persistent problem, device graph construction, the Ceres-compatible
// Levenberg-Marquardt trust-region controller (its PCG: pgo_pcg.hip), optional RCCL edge sharding, and the C-ABI (include/pgo.h).
//
// What it replaces in the reference: the `ceres::Problem` bookkeeping calls of
// PoseGraphSLAM::reinit_ceres_problem_onnewloopedge_optimize6DOF (src/PoseGraphSLAM.cpp:1340-1367,1550-1556,
// 1629-1633,1803-1849) and `ceres::Solve` (:1903) with the options at :1268-1272.  The minimiser follows
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

// scalar slots
enum { S_COST = 0, S_PRIOR_COST = 1, S_MODEL = 2, S_SW_STEP2 = 3, S_SW_XNORM2 = 4, S_GMAX = 5, S_STEP2 = 6, S_XNORM2 = 7, S_N = 8 };

int set_device(pgo_problem* p) { HIPCHK(p, hipSetDevice(p->device)); return PGO_OK; }

// Matrix4d (column-major 16) -> Meas fields
void meas_from_matrix(const double* T, double w, double* out8) {
    double R[9];
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) R[r * 3 + c] = T[c * 4 + r];
    double q[4];
    eigen_matrix_to_quat(R, q);   // CeresResidues.h:24 / :150
    out8[0] = q[0]; out8[1] = q[1]; out8[2] = q[2]; out8[3] = q[3];
    out8[4] = T[12]; out8[5] = T[13]; out8[6] = T[14]; out8[7] = w;
}

int upload_class(pgo_problem* p, const HostClass& H, bool is_sw, DBuf<int32_t>& dc1, DBuf<int32_t>& dc2, DBuf<int32_t>& dsw, DBuf<double>& dmeas,
                 DBuf<int4>& dwin, EdgeClassDev& out) {
    const int32_t* g2l = p->local_ids ? p->g2l.data() : nullptr;
    const int64_t E = H.size();
    const int64_t Epad = (E + TILE - 1) / TILE * TILE;
    const int tiles = (int)(Epad / TILE);
    std::vector<int32_t> c1(Epad), c2(Epad), sw(is_sw ? Epad : 0);
    std::vector<double> meas((size_t)8 * Epad);
    std::vector<int4> win(tiles);
    for (int64_t e = 0; e < Epad; ++e) {
        const int64_t s = e < E ? e : E - 1;   // padding lanes replicate the last edge (computed, never stored or counted)
        c1[e] = g2l ? g2l[H.c1[s]] : H.c1[s]; c2[e] = g2l ? g2l[H.c2[s]] : H.c2[s];
        if (is_sw) sw[e] = H.sw[s];
        for (int k = 0; k < 8; ++k) meas[(size_t)k * Epad + e] = H.meas[(size_t)s * 8 + k];
    }
    for (int t = 0; t < tiles; ++t) {
        int lo1 = INT32_MAX, hi1 = -1, lo2 = INT32_MAX, hi2 = -1;
        for (int l = 0; l < TILE; ++l) {
            const int64_t e = (int64_t)t * TILE + l;
            lo1 = std::min(lo1, c1[e]); hi1 = std::max(hi1, c1[e]); lo2 = std::min(lo2, c2[e]); hi2 = std::max(hi2, c2[e]);
        }
        const int n1 = hi1 - lo1 + 1, n2 = hi2 - lo2 + 1;
        win[t] = make_int4(lo1, n1 <= WIN_MAX ? n1 : 0, lo2, n2 <= WIN_MAX ? n2 : 0);
    }
    if (Epad > 0) {
        HIPCHK(p, dc1.ensure(Epad)); HIPCHK(p, dc2.ensure(Epad)); HIPCHK(p, dmeas.ensure((size_t)8 * Epad)); HIPCHK(p, dwin.ensure(tiles));
        HIPCHK(p, hipMemcpyAsync(dc1.p, c1.data(), Epad * sizeof(int32_t), hipMemcpyHostToDevice, p->st));
        HIPCHK(p, hipMemcpyAsync(dc2.p, c2.data(), Epad * sizeof(int32_t), hipMemcpyHostToDevice, p->st));
        HIPCHK(p, hipMemcpyAsync(dmeas.p, meas.data(), (size_t)8 * Epad * sizeof(double), hipMemcpyHostToDevice, p->st));
        HIPCHK(p, hipMemcpyAsync(dwin.p, win.data(), tiles * sizeof(int4), hipMemcpyHostToDevice, p->st));
        if (is_sw) { HIPCHK(p, dsw.ensure(Epad)); HIPCHK(p, hipMemcpyAsync(dsw.p, sw.data(), Epad * sizeof(int32_t), hipMemcpyHostToDevice, p->st)); }
        HIPCHK(p, hipStreamSynchronize(p->st));   // host vectors die at scope exit
    }
    out.c1 = dc1.p; out.c2 = dc2.p; out.meas = dmeas.p; out.swidx = is_sw ? dsw.p : nullptr; out.win = dwin.p;
    out.E = E; out.Epad = Epad; out.tiles = tiles; out.J = nullptr;
    return PGO_OK;
}

}  // namespace

namespace pgo {

// several ranks: send / receive buffers for the largest exchange of the handle — 42 doubles per row of the keyframes' plan (diagonal block + gradient), 12 per row of a
// level plan (x and r of a level travel together).  Two send buffers: the in-process communicator double-buffers by collective parity.
int ensure_exchange_buffers(pgo_problem* p) {
    if (!p->local_ids) return PGO_OK;
    size_t ns = (size_t)p->fine_plan.x.n_send() * 42, nr = (size_t)p->fine_plan.x.n_recv() * 42;
    for (const LevelPlanDev& L : p->mg.lvl_plan) if (L.plan) { ns = std::max(ns, (size_t)L.plan->n_send() * 12); nr = std::max(nr, (size_t)L.plan->n_recv() * 12); }
    if (p->mg.first_whole > 0) {      // distributed set-up: 36 doubles per block of the levels, of Ps and per row of Dinv (the level plans), 18 per fp32 block of R
        for (int l = 0; l < p->mg.first_whole && (size_t)l < p->mg.lvl_plan.size(); ++l) if (p->mg.lvl_plan[(size_t)l].plan) { ns = std::max(ns, (size_t)p->mg.lvl_plan[(size_t)l].plan->n_send() * 36); nr = std::max(nr, (size_t)p->mg.lvl_plan[(size_t)l].plan->n_recv() * 36); }
        for (const pgo_mg::BlockPlan& B : p->mg.setup.val) { ns = std::max(ns, (size_t)B.x.n_send() * 36); nr = std::max(nr, (size_t)B.x.n_recv() * 36); }
        for (const pgo_mg::ExchangePlan& X : p->mg.setup.ps) { ns = std::max(ns, (size_t)X.n_send() * 36); nr = std::max(nr, (size_t)X.n_recv() * 36); }
        for (const pgo_mg::ExchangePlan& X : p->mg.setup.rv) { ns = std::max(ns, (size_t)X.n_send() * 18); nr = std::max(nr, (size_t)X.n_recv() * 18); }
    }
    HIPCHK(p, p->d_xsend[0].ensure(ns + 64)); HIPCHK(p, p->d_xsend[1].ensure(ns + 64)); HIPCHK(p, p->d_xrecv.ensure(nr + 64)); HIPCHK(p, p->d_xscal.ensure(16));
    return PGO_OK;
}

}  // namespace pgo

namespace {

int build_graph(pgo_problem* p, int64_t N, int64_t S, const double* sw_now) {
    mg_drop_pending(p);      // (a worker reads the host arrays rebuilt below)
    double t_phase = now_s();
    auto phase = [&](const char* what) { if (p->opt.verbosity > 1) { const double t = now_s(); std::fprintf(stderr, "[pgo] build_graph: %-34s %7.2f ms\n", what, (t - t_phase) * 1e3); t_phase = t; } };
    // ---- validate against the array sizes the caller solves with
    for (const HostClass* H : {&p->rel, &p->swe})
        for (int64_t e = 0; e < H->size(); ++e)
            if (H->c1[e] < 0 || H->c1[e] >= N || H->c2[e] < 0 || H->c2[e] >= N) { p->err = "edge endpoint out of range for n_nodes"; return PGO_ERR_INVALID_ARG; }
    p->h_sw_used.assign((size_t)S, 0);
    for (int64_t e = 0; e < p->swe.size(); ++e) {
        const int32_t si = p->swe.sw[e];
        if (si < 0 || si >= S) { p->err = "switch index out of range for n_switch"; return PGO_ERR_INVALID_ARG; }
        if (p->h_sw_used[si]) { p->err = "switch index used by more than one edge"; return PGO_ERR_INVALID_ARG; }
        p->h_sw_used[si] = 1;
    }
    for (const PriorDev& pr : p->priors) if (pr.node < 0 || pr.node >= N) { p->err = "regulariser node out of range"; return PGO_ERR_INVALID_ARG; }
    p->S = S; p->N_global = N;
    GraphDev& G = p->G;
    G = GraphDev{};
    // ---- multi-GPU: rank-local subgraph.  This rank works on the keyframes its own residual blocks touch, renumbered densely; keyframes
    // touched by >= 2 ranks are "shared" (their rows are summed over ranks by exchange_rows), the lowest touching rank is the owner.
    const int64_t Ng = N;
    p->local_ids = p->comm != nullptr;   // also with a 1-rank communicator: the same code path, every collective issued
    p->n_sh_mine = p->n_sh_global = 0;
    if (p->local_ids) {
        std::vector<uint8_t> touched((size_t)Ng, 0);
        std::vector<int32_t> deg((size_t)Ng, 0);      // residual blocks of THIS rank on each keyframe
        for (const HostClass* H : {&p->rel, &p->swe}) for (int64_t e = 0; e < H->size(); ++e) { touched[H->c1[e]] = 1; touched[H->c2[e]] = 1; ++deg[H->c1[e]]; ++deg[H->c2[e]]; }
        for (const PriorDev& pr : p->priors) { touched[pr.node] = 1; ++deg[pr.node]; }
        bool any = false;
        for (int64_t g = 0; g < Ng && !any; ++g) any = touched[g] != 0;
        if (!any) touched[0] = 1;   // a rank without residual blocks still takes part in every collective: give it one (zero-contribution) keyframe
        // Two all-reduces of Ng doubles, once per graph build.  Sum: every rank adds 2^rank for the keyframes it touches — the set of touching ranks (exact in a double up to
        // 52 ranks): how many they are, and who exchanges the keyframe's rows with whom.  Max of (blocks + 1) * 64 + 63 - rank: the OWNER — the rank holding most of the
        // keyframe's residual blocks, the lowest of them on a tie (pgo_mg_host.hpp: Owners).
        if (p->world() > 52) { p->err = "more than 52 ranks"; return PGO_ERR_INVALID_ARG; }
        std::vector<double> buf((size_t)Ng), obuf((size_t)Ng);
        for (int64_t g = 0; g < Ng; ++g) { buf[g] = touched[g] ? std::ldexp(1.0, p->rank()) : 0.0; obuf[g] = touched[g] ? (double)(((int64_t)deg[g] + 1) * 64 + 63 - p->rank()) : 0.0; }
        int rc2;
        if ((rc2 = host_allreduce(p, buf, 0)) != PGO_OK) return rc2;
        if ((rc2 = host_allreduce(p, obuf, 2)) != PGO_OK) return rc2;
        p->h_touch_mask.assign((size_t)Ng, 0); p->h_owner.assign((size_t)Ng, -1);
        p->l2g.clear(); p->g2l.assign((size_t)Ng, -1); p->h_own.clear(); p->h_touched_any.assign((size_t)Ng, 0);
        int64_t pos = 0, n_mine = 0;
        for (int64_t g = 0; g < Ng; ++g) {
            const uint64_t m = (uint64_t)(buf[g] + 0.5);
            p->h_touch_mask[g] = m;
            const int cnt = __builtin_popcountll(m);
            if (m) { p->h_owner[g] = 63 - (int32_t)((int64_t)(obuf[g] + 0.5) % 64); if (!((m >> p->h_owner[g]) & 1)) { p->err = "graph build: a keyframe's owner does not touch it (the ranks' all-reduces disagree)"; return PGO_ERR_COMM; } }
            p->h_touched_any[g] = cnt > 0;
            if (touched[g]) {
                if (!((m >> p->rank()) & 1)) { p->err = "touch masks: the all-reduce did not return this rank's own bit"; return PGO_ERR_COMM; }
                p->g2l[g] = (int32_t)p->l2g.size();
                if (cnt >= 2) ++n_mine;
                p->l2g.push_back((int32_t)g);
                p->h_own.push_back(p->h_owner[g] == p->rank() ? 1.0 : 0.0);
            }
            if (cnt >= 2) ++pos;
        }
        p->n_sh_global = pos; p->n_sh_mine = n_mine;
        N = (int64_t)p->l2g.size();
        HIPCHK(p, p->d_l2g.ensure(N)); HIPCHK(p, p->d_own.ensure(N));
        HIPCHK(p, hipMemcpyAsync(p->d_l2g.p, p->l2g.data(), N * sizeof(int32_t), hipMemcpyHostToDevice, p->st));
        HIPCHK(p, hipMemcpyAsync(p->d_own.p, p->h_own.data(), N * sizeof(double), hipMemcpyHostToDevice, p->st));
        {   // the keyframes' neighbour exchange: segments per peer, and for every shared keyframe the order its parts are summed in (pgo_mg_host.hpp: build_fine_plan)
            pgo_mg::build_fine_plan(p->h_touch_mask, p->l2g, p->rank(), p->world(), p->fine_plan);
            const pgo_mg::FinePlan& F = p->fine_plan;
            auto up = [&](DBuf<int32_t>& d, const std::vector<int32_t>& v) -> int {
                HIPCHK(p, d.ensure(std::max<size_t>(v.size(), 1)));
                if (!v.empty()) HIPCHK(p, hipMemcpyAsync(d.p, v.data(), v.size() * sizeof(int32_t), hipMemcpyHostToDevice, p->st));
                return PGO_OK;
            };
            if ((rc2 = up(p->d_fp_send, F.x.send_idx)) != PGO_OK || (rc2 = up(p->d_fp_shloc, F.sh_loc)) != PGO_OK || (rc2 = up(p->d_fp_sumptr, F.sum_ptr)) != PGO_OK || (rc2 = up(p->d_fp_sumsrc, F.sum_src)) != PGO_OK) return rc2;
            p->mg.lvl_plan.clear();
            if ((rc2 = ensure_exchange_buffers(p)) != PGO_OK) return rc2;
        }
        HIPCHK(p, hipStreamSynchronize(p->st));
        G.own = p->d_own.p;
    } else {
        p->l2g.clear(); p->g2l.clear(); p->h_own.clear(); p->h_touched_any.clear();
        G.own = nullptr;
    }
    p->N = N;
    phase("validation, rank-local numbering");
    const int32_t* g2l = p->local_ids ? p->g2l.data() : nullptr;
    auto L = [g2l](int32_t g) -> int32_t { return g2l ? g2l[g] : g; };
    G.N = N; G.S = S;
    int rc;
    // a keyframe is part of the program when a residual block touches it: on one GPU that is a non-empty incident list; in a rank-local
    // subgraph every keyframe is touched by construction (by this rank or, for the stand-in keyframe of an idle rank, possibly by none)
    p->h_node_free.assign((size_t)N, 0);
    {
        std::vector<uint8_t> touched_here((size_t)N, 0);      // (= a non-empty incident list, known before the lists are built: the hierarchy worker below starts at once)
        for (const HostClass* H : {&p->rel, &p->swe}) for (int64_t e = 0; e < H->size(); ++e) { touched_here[L(H->c1[e])] = 1; touched_here[L(H->c2[e])] = 1; }
        for (const PriorDev& pr : p->priors) touched_here[L(pr.node)] = 1;
        for (int64_t n = 0; n < N; ++n) p->h_node_free[n] = (touched_here[n] || (p->local_ids && p->h_touched_any[p->l2g[n]])) ? 1 : 0;
    }
    for (int32_t c : p->constant_nodes) if (c >= 0 && c < Ng && L(c) >= 0) p->h_node_free[L(c)] = 0;
    // One GPU: the HOST half of the multigrid hierarchy (pgo_mg_host.hpp: ~0.1 s for C3, single-threaded sorts and matchings) needs the edge lists and the free flags
    // only, so it runs on a worker thread beside the rest of this function — incident-list upload, matrix-free tile packing, buffer allocation — and is installed where
    // build_multigrid used to compute it.  Nothing here depends on timing: the result is the same hierarchy.  (Several ranks: its host half holds collectives.)
    struct Guard { pgo_problem* p; bool committed = false; ~Guard() { if (!committed) mg_drop_pending(p); } } mg_guard{p};     // an early return below waits for the worker and drops its result
    mg_start_fresh(p, sw_now);
    if ((rc = upload_class(p, p->rel, false, p->d_rc1, p->d_rc2, p->d_sidx /*unused*/, p->d_rmeas, p->d_rwin, G.rel)) != PGO_OK) return rc;
    if ((rc = upload_class(p, p->swe, true, p->d_sc1, p->d_sc2, p->d_sidx, p->d_smeas, p->d_swin, G.sw)) != PGO_OK) return rc;
    const int64_t Er = G.rel.E, Es = G.sw.E, Eg = (int64_t)p->priors.size();
    phase("edge classes packed + uploaded");
    std::vector<PriorDev> pri = p->priors;
    for (PriorDev& x : pri) x.node = L(x.node);
    // ---- node -> incident list (edges in slot order, then regularisers), BSR structure
    std::vector<int64_t> rowptr(N + 1, 0), bsr_rowptr(N + 1, 0);
    for (int64_t e = 0; e < Er; ++e) { rowptr[L(p->rel.c1[e]) + 1]++; rowptr[L(p->rel.c2[e]) + 1]++; }
    for (int64_t e = 0; e < Es; ++e) { rowptr[L(p->swe.c1[e]) + 1]++; rowptr[L(p->swe.c2[e]) + 1]++; }
    for (int64_t n = 0; n < N; ++n) bsr_rowptr[n + 1] = bsr_rowptr[n] + 1 + rowptr[n + 1];
    for (int64_t k = 0; k < Eg; ++k) rowptr[pri[k].node + 1]++;
    for (int64_t n = 0; n < N; ++n) rowptr[n + 1] += rowptr[n];
    const int64_t ninc = rowptr[N];
    p->nnzb = bsr_rowptr[N];
    std::vector<int64_t> inc((size_t)ninc), fill(rowptr.begin(), rowptr.end() - 1);
    std::vector<int32_t> bsr_col((size_t)p->nnzb);
    std::vector<int64_t> bfill(N);
    for (int64_t n = 0; n < N; ++n) { bsr_col[bsr_rowptr[n]] = (int32_t)n; bfill[n] = bsr_rowptr[n] + 1; }
    auto add_edge = [&](int64_t slot, int32_t a, int32_t b) {
        inc[fill[a]++] = (slot << 1) | 0; bsr_col[bfill[a]++] = b;
        inc[fill[b]++] = (slot << 1) | 1; bsr_col[bfill[b]++] = a;
    };
    for (int64_t e = 0; e < Er; ++e) add_edge(e, L(p->rel.c1[e]), L(p->rel.c2[e]));
    for (int64_t e = 0; e < Es; ++e) add_edge(G.rel.Epad + e, L(p->swe.c1[e]), L(p->swe.c2[e]));
    for (int64_t k = 0; k < Eg; ++k) inc[fill[pri[k].node]++] = ((G.rel.Epad + G.sw.Epad + k) << 1);

    HIPCHK(p, p->d_inc_rowptr.ensure(N + 1)); HIPCHK(p, p->d_bsr_rowptr.ensure(N + 1)); HIPCHK(p, p->d_inc.ensure(std::max<int64_t>(ninc, 1)));
    HIPCHK(p, p->d_bsr_col.ensure(std::max<int64_t>(p->nnzb, 1))); HIPCHK(p, p->d_node_free.ensure(std::max<int64_t>(N, 1)));
    HIPCHK(p, p->d_prior.ensure(std::max<int64_t>(Eg, 1)));
    HIPCHK(p, hipMemcpyAsync(p->d_inc_rowptr.p, rowptr.data(), (N + 1) * sizeof(int64_t), hipMemcpyHostToDevice, p->st));
    HIPCHK(p, hipMemcpyAsync(p->d_bsr_rowptr.p, bsr_rowptr.data(), (N + 1) * sizeof(int64_t), hipMemcpyHostToDevice, p->st));
    if (ninc) HIPCHK(p, hipMemcpyAsync(p->d_inc.p, inc.data(), ninc * sizeof(int64_t), hipMemcpyHostToDevice, p->st));
    if (p->nnzb) HIPCHK(p, hipMemcpyAsync(p->d_bsr_col.p, bsr_col.data(), p->nnzb * sizeof(int32_t), hipMemcpyHostToDevice, p->st));
    if (N) HIPCHK(p, hipMemcpyAsync(p->d_node_free.p, p->h_node_free.data(), N, hipMemcpyHostToDevice, p->st));
    if (Eg) HIPCHK(p, hipMemcpyAsync(p->d_prior.p, pri.data(), Eg * sizeof(PriorDev), hipMemcpyHostToDevice, p->st));
    HIPCHK(p, hipStreamSynchronize(p->st));

    phase("incident lists + block-CSR structure");
    // ---- matrix-free operator: edge-sides in keyframe-major order, packed into workgroup tiles of whole keyframes
    bool mf = p->opt.linear_solver == PGO_LINEAR_PCG_MATRIX_FREE;
    if (mf) {
        // a keyframe with more edge sides than a workgroup tile holds (a hub revisited hundreds of times), or with several regularisers,
        // is served by the assembled block-CSR operator instead
        const int64_t slot_pr0 = G.rel.Epad + G.sw.Epad;
        for (int64_t n = 0; n < N && mf; ++n) {
            int64_t deg = 0, npri = 0;
            for (int64_t k = rowptr[n]; k < rowptr[n + 1]; ++k) { if ((inc[k] >> 1) >= slot_pr0) ++npri; else ++deg; }
            if (deg > MF_BLOCK || npri > 1) mf = false;
        }
    }
    p->built_mf = mf;
    p->F = MfDev{};
    if (mf) {
        // per keyframe: its relative-pose sides and its switchable sides (both in incident-list order), regulariser index
        std::vector<int32_t> node_prior(N, -1), deg_rel(N, 0), deg_sw(N, 0);
        const int64_t slot_pr = G.rel.Epad + G.sw.Epad;
        for (int64_t n = 0; n < N; ++n) {
            for (int64_t k = rowptr[n]; k < rowptr[n + 1]; ++k) {
                const int64_t slot = inc[k] >> 1;
                if (slot >= slot_pr) {
                    if (node_prior[n] >= 0) { p->err = "matrix-free operator: more than one regulariser on a keyframe"; return PGO_ERR_INVALID_ARG; }
                    node_prior[n] = (int32_t)(slot - slot_pr);
                } else if (slot >= G.rel.Epad) ++deg_sw[n]; else ++deg_rel[n];
            }
            if (deg_rel[n] + deg_sw[n] > MF_BLOCK) { p->err = "matrix-free operator: a keyframe with more incident edges than a matrix-free tile holds (use PGO_LINEAR_PCG_BLOCK_JACOBI)"; return PGO_ERR_INVALID_ARG; }
        }
        if ((int64_t)std::max(G.rel.E, G.sw.E) >= (1ll << 30)) { p->err = "matrix-free operator: more than 2^30 edges in one class"; return PGO_ERR_INVALID_ARG; }
        // pack whole keyframes into workgroup tiles: <= MF_SLOTS edge sides, <= MF_BLOCK lanes (a relative-pose edge with both keyframes in
        // the tile takes ONE lane for its two sides), <= MF_MAX_NODES keyframes
        auto rel_other_of = [&](int64_t k) -> int32_t {      // incident entry k of a relative-pose side: the other keyframe, or -1
            const int64_t slot = inc[k] >> 1; const int side = (int)(inc[k] & 1);
            if (slot >= G.rel.Epad) return -1;
            const int32_t a = L(p->rel.c1[slot]), b = L(p->rel.c2[slot]);
            return a == b ? -1 : (side == 0 ? b : a);
        };
        std::vector<int32_t> tile_node0; tile_node0.push_back(0);
        { int64_t sides = 0, pairs = 0; int cur_nodes = 0; int32_t start = 0;
          for (int64_t n = 0; n < N; ++n) {
              const int64_t d = deg_rel[n] + deg_sw[n];
              auto pairs_with = [&](int32_t lo) { int64_t c = 0; for (int64_t k = rowptr[n]; k < rowptr[n + 1]; ++k) { const int32_t o = rel_other_of(k); if (o >= lo && o < (int32_t)n) ++c; } return c; };
              int64_t np = pairs_with(start);
              if (sides + d > MF_SLOTS || sides + d - (pairs + np) > MF_BLOCK || cur_nodes >= MF_MAX_NODES) {
                  tile_node0.push_back((int32_t)n); sides = 0; pairs = 0; cur_nodes = 0; start = (int32_t)n; np = 0;
              }
              sides += d; pairs += np; ++cur_nodes;
          }
          tile_node0.push_back((int32_t)N); }
        const int tiles = (int)tile_node0.size() - 1;
        std::vector<int64_t> tile_inc0(tiles + 1, 0);
        std::vector<int32_t> tile_sw0(std::max(tiles, 1), 0);
        std::vector<uint32_t> einc, eslot; std::vector<int32_t> eoth; std::vector<ushort4> node_rng(std::max<int64_t>(N, 1));
        einc.reserve((size_t)(Er + 2 * Es) + 64); eoth.reserve(einc.capacity()); eslot.reserve(einc.capacity());
        std::vector<uint16_t> side_slot((size_t)(rowptr[N]), 0);       // slot of incident entry k inside its tile
        std::vector<uint16_t> rel_slot1((size_t)std::max<int64_t>(Er, 1), 0);   // per relative-pose edge: slot of its side 1 (own = c2)
        for (int t = 0; t < tiles; ++t) {
            const int32_t n0 = tile_node0[t], n1 = tile_node0[t + 1];
            tile_inc0[t] = (int64_t)einc.size();
            // slots: the keyframes' relative-pose sides, then their switchable sides, each in incident-list order
            int slot_n = 0;
            for (int pass = 0; pass < 2; ++pass)
                for (int32_t n = n0; n < n1; ++n) {
                    const unsigned short begin = (unsigned short)slot_n;
                    for (int64_t k = rowptr[n]; k < rowptr[n + 1]; ++k) {
                        const int64_t slot = inc[k] >> 1;
                        if (slot >= slot_pr || (int)(slot >= G.rel.Epad) != pass) continue;
                        side_slot[k] = (uint16_t)slot_n;
                        if (pass == 0 && (inc[k] & 1)) rel_slot1[slot] = (uint16_t)slot_n;
                        ++slot_n;
                    }
                    if (pass == 0) { node_rng[n].x = begin; node_rng[n].y = (unsigned short)slot_n; } else { node_rng[n].z = begin; node_rng[n].w = (unsigned short)slot_n; }
                }
            // lanes: pairs, then the other relative-pose sides, then the switchable sides
            int n_pairs = 0;
            for (int group = 0; group < 3; ++group) {
                if (group == 2) tile_sw0[t] = (int32_t)(((int64_t)einc.size() - tile_inc0[t]) | ((int64_t)n_pairs << 16));
                for (int32_t n = n0; n < n1; ++n)
                    for (int64_t k = rowptr[n]; k < rowptr[n + 1]; ++k) {
                        const int64_t slot = inc[k] >> 1; const int side = (int)(inc[k] & 1);
                        if (slot >= slot_pr) continue;
                        const bool is_sw = slot >= G.rel.Epad;
                        if (is_sw != (group == 2)) continue;
                        const int64_t e = is_sw ? slot - G.rel.Epad : slot;
                        const int32_t a = L(is_sw ? p->swe.c1[e] : p->rel.c1[e]), b = L(is_sw ? p->swe.c2[e] : p->rel.c2[e]);
                        const int32_t other = side == 0 ? b : a;
                        const bool paired = !is_sw && a != b && other >= n0 && other < n1;
                        if (group == 0) {
                            if (!paired || side != 0) continue;          // the pair's lane stands at side 0 (own = c1)
                            einc.push_back((uint32_t)(e << 1));
                            eoth.push_back(b);
                            eslot.push_back((uint32_t)side_slot[k] | ((uint32_t)rel_slot1[e] << 9) | ((uint32_t)(n - n0) << 18));
                            ++n_pairs;
                        } else {
                            if (group == 1 && paired) continue;
                            einc.push_back((is_sw ? 0x80000000u : 0u) | (uint32_t)(e << 1) | (uint32_t)side);
                            eoth.push_back(other);
                            eslot.push_back((uint32_t)side_slot[k] | (511u << 9) | ((uint32_t)(n - n0) << 18));
                        }
                    }
            }
        }
        tile_inc0[tiles] = (int64_t)einc.size();
        p->mf_pair_lanes = 0; p->mf_sw_lanes = 0;
        for (int t = 0; t < tiles; ++t) { p->mf_pair_lanes += (uint32_t)tile_sw0[t] >> 16; p->mf_sw_lanes += (tile_inc0[t + 1] - tile_inc0[t]) - (tile_sw0[t] & 0xffff); }
        p->mf_rel_side_lanes = (int64_t)einc.size() - p->mf_pair_lanes - p->mf_sw_lanes;
        const int64_t ninc_e = (int64_t)einc.size();
        const int64_t ninc_pad = (ninc_e + 63) / 64 * 64 + 64;
        HIPCHK(p, p->d_einc.ensure(std::max<int64_t>(ninc_e, 1))); HIPCHK(p, p->d_einc_slot.ensure(std::max<int64_t>(ninc_e, 1))); HIPCHK(p, p->d_einc_other.ensure(std::max<int64_t>(ninc_e, 1)));
        HIPCHK(p, p->d_node_rng.ensure(std::max<int64_t>(N, 1))); HIPCHK(p, p->d_tile_inc0.ensure(tiles + 1)); HIPCHK(p, p->d_tile_node0.ensure(tiles + 1));
        HIPCHK(p, p->d_tile_sw0.ensure(std::max(tiles, 1))); HIPCHK(p, p->d_node_prior.ensure(std::max<int64_t>(N, 1)));
        HIPCHK(p, p->d_rec.ensure((size_t)MF_PLANES * ninc_pad)); HIPCHK(p, p->d_lam.ensure(std::max<int64_t>(N * 6, 1)));
        if (ninc_e) {
            HIPCHK(p, hipMemcpyAsync(p->d_einc.p, einc.data(), ninc_e * sizeof(uint32_t), hipMemcpyHostToDevice, p->st));
            HIPCHK(p, hipMemcpyAsync(p->d_einc_slot.p, eslot.data(), ninc_e * sizeof(uint32_t), hipMemcpyHostToDevice, p->st));
            HIPCHK(p, hipMemcpyAsync(p->d_einc_other.p, eoth.data(), ninc_e * sizeof(int32_t), hipMemcpyHostToDevice, p->st));
        }
        HIPCHK(p, hipMemcpyAsync(p->d_node_rng.p, node_rng.data(), N * sizeof(ushort4), hipMemcpyHostToDevice, p->st));
        HIPCHK(p, hipMemcpyAsync(p->d_tile_inc0.p, tile_inc0.data(), (tiles + 1) * sizeof(int64_t), hipMemcpyHostToDevice, p->st));
        HIPCHK(p, hipMemcpyAsync(p->d_tile_node0.p, tile_node0.data(), (tiles + 1) * sizeof(int32_t), hipMemcpyHostToDevice, p->st));
        if (tiles) HIPCHK(p, hipMemcpyAsync(p->d_tile_sw0.p, tile_sw0.data(), tiles * sizeof(int32_t), hipMemcpyHostToDevice, p->st));
        HIPCHK(p, hipMemcpyAsync(p->d_node_prior.p, node_prior.data(), N * sizeof(int32_t), hipMemcpyHostToDevice, p->st));
        HIPCHK(p, hipStreamSynchronize(p->st));
        p->F = MfDev{p->d_einc.p, p->d_einc_other.p, p->d_einc_slot.p, p->d_tile_inc0.p, p->d_tile_sw0.p, p->d_tile_node0.p, p->d_node_rng.p, p->d_node_prior.p,
                     p->d_rec.p, p->d_lam.p, ninc_e, ninc_pad, tiles};
    }
    phase("matrix-free tiles");
    // ---- work buffers
    const int64_t slots = G.rel.Epad + G.sw.Epad;
    HIPCHK(p, p->d_Jr.ensure(std::max<int64_t>((int64_t)G.rel.tiles * REL_DOUBLES * TILE, 1)));
    HIPCHK(p, p->d_Js.ensure(std::max<int64_t>((int64_t)G.sw.tiles * SW_DOUBLES * TILE, 1)));
    HIPCHK(p, p->d_Jp.ensure(std::max<int64_t>(Eg * PRIOR_DOUBLES, 1)));
    HIPCHK(p, p->d_Hd_g.ensure(std::max<int64_t>(N * 42, 1)));
    HIPCHK(p, p->d_Hoff.ensure(mf ? 1 : std::max<int64_t>(slots * 36, 1)));
    HIPCHK(p, p->d_c.ensure(std::max<int64_t>(Es * 12, 1))); HIPCHK(p, p->d_hss.ensure(std::max<int64_t>(Es, 1))); HIPCHK(p, p->d_gs.ensure(std::max<int64_t>(Es, 1)));
    HIPCHK(p, p->d_scale_p.ensure(std::max<int64_t>(N * 6, 1))); HIPCHK(p, p->d_diag_p.ensure(std::max<int64_t>(N * 6, 1)));
    HIPCHK(p, p->d_scale_s.ensure(std::max<int64_t>(Es, 1))); HIPCHK(p, p->d_diag_s.ensure(std::max<int64_t>(Es, 1))); HIPCHK(p, p->d_a_inv.ensure(std::max<int64_t>(Es, 1)));
    HIPCHK(p, p->d_val.ensure(mf ? 1 : std::max<int64_t>(p->nnzb * 36, 1))); HIPCHK(p, p->d_Lf.ensure(std::max<int64_t>(N * 24 + 64 * 24, 1))); HIPCHK(p, p->d_Dtot_b.ensure(std::max<int64_t>(N * 42, 1)));
    HIPCHK(p, p->d_cgvec.ensure(std::max<int64_t>(N * 42, 1)));
    p->n_part = std::max<int64_t>(MAX_PARTIALS, (G.rel.tiles + G.sw.tiles + 3) / 4 + 1);
    HIPCHK(p, p->d_part.ensure(p->n_part * 6));
    HIPCHK(p, p->d_cgpart.ensure(PQ_SLOTS + 2 * RZ_STRIDE + 16));   // partial sums + 16 PCG scalars (C.scal)
    HIPCHK(p, p->d_flags.ensure(8)); HIPCHK(p, p->d_scal.ensure(S_N));
    for (int k = 0; k < 2; ++k) { HIPCHK(p, p->d_pose[k].ensure(std::max<int64_t>(N * 8, 1))); HIPCHK(p, p->d_swv[k].ensure(std::max<int64_t>(S, 1))); }
    HIPCHK(p, p->d_delta_s.ensure(std::max<int64_t>(Es, 1))); HIPCHK(p, p->d_io.ensure(std::max<int64_t>(N * 7, 1)));

    G.rel.J = p->d_Jr.p; G.sw.J = p->d_Js.p;
    G.prior = p->d_prior.p; G.n_prior = (int32_t)Eg; G.Jp = p->d_Jp.p;
    G.inc_rowptr = p->d_inc_rowptr.p; G.inc = p->d_inc.p; G.node_free = p->d_node_free.p;
    G.bsr_rowptr = p->d_bsr_rowptr.p; G.bsr_col = p->d_bsr_col.p; G.nnzb = p->nnzb;
    p->L = LinDev{p->d_Hd_g.p, p->d_Hd_g.p + (size_t)N * 36, p->d_Hoff.p, p->d_c.p, p->d_hss.p, p->d_gs.p};
    p->Sc = ScaleDev{p->d_scale_p.p, p->d_scale_s.p, p->d_diag_p.p, p->d_diag_s.p, p->d_a_inv.p};
    CgDev& C = p->C;
    C.val = p->d_val.p; C.Lf = p->d_Lf.p; C.Dtot = p->d_Dtot_b.p; C.b = p->d_Dtot_b.p + (size_t)N * 36;
    double* v = p->d_cgvec.p; const size_t n6 = (size_t)N * 6;
    C.x = v; C.r = v + n6; C.r2 = v + 2 * n6; C.z = v + 3 * n6; C.p = v + 4 * n6; C.p2 = v + 5 * n6; C.q = v + 6 * n6;
    C.part_pq = p->d_cgpart.p; C.part_rz = p->d_cgpart.p + PQ_SLOTS; C.scal = p->d_cgpart.p + PQ_SLOTS + 2 * RZ_STRIDE; C.extra_rz = 0;
    C.flags = p->d_flags.p;
    // ---- aggregation multigrid for large graphs: hierarchy of graph-following rigid aggregates (pgo_mg_host.hpp), built by build_multigrid() below — which a solve
    // may call again with the current switch values (regroup)
    phase("work buffers");
    if ((rc = build_multigrid(p, sw_now)) != PGO_OK) return rc;      // (one GPU: only announced, the hierarchy is on the worker)
    phase("multigrid hierarchy");
    if (p->mg.built && p->built_mf) { HIPCHK(p, p->d_Hoff.ensure((size_t)(p->G.rel.Epad + p->G.sw.Epad) * 36)); p->L.Hoff = p->d_Hoff.p; }      // the multigrid's level-1 product reads J1^T J2 per edge
    p->hoff_epoch = 0;
    if (!p->mg.built && (rc = build_two_level_aggregates(p)) != PGO_OK) return rc;      // (a graph that got the multigrid never uses the two-level method: its dense operator would be built and uploaded for nothing)
    phase("two-level aggregates");
    mg_guard.committed = true;
    p->graph_dirty = false; p->priors_dirty = false;
    ++p->pcg.build_epoch;   // invalidates the captured PCG graph (kernel arguments hold device pointers / sizes)
    return PGO_OK;
}

}  // namespace

namespace pgo {

// ---- collectives (no-ops without a communicator; a 1-rank communicator still issues every call) ----
// a graph built for several ranks whose communicator has gone since (pgo_comm_destroy inside a solve): its collectives fail
static int no_comm(pgo_problem* p) { p->err = "no communicator: the graph was built for several ranks (pgo_comm_destroy inside a solve?)"; return PGO_ERR_STATE; }
int allreduce(pgo_problem* p, double* buf, size_t n, int op /*0 sum, 2 max*/) {
    if (!p->comm) return p->local_ids ? no_comm(p) : PGO_OK;
    ++p->st_allreduces; p->st_bytes_allreduce += (double)n * sizeof(double);
    return p->comm->allreduce(buf, n, op, p->err);
}

// Neighbour exchange of `K` doubles per row (pgo_comm.hpp: Comm::exchange): `pack` fills the send buffer the transport hands out, `unpack` reads the receive buffer
template <class Pack, class Unpack>
static int neighbor_exchange(pgo_problem* p, const pgo_mg::ExchangePlan& X, int K, Pack pack, Unpack unpack) {
    if (!p->comm) return no_comm(p);
    const int slot = p->comm->send_slot(p->err);
    if (slot < 0) return slot;
    pack(p->d_xsend[slot].p);
    ++p->st_exchanges; p->st_bytes_neighbour += (double)X.n_send() * K * sizeof(double);
    size_t reduced = 0;      // (an exchange emulated by an all-reduce counts as one as well)
    const int rc = p->comm->exchange({X.send_off.data(), X.recv_off.data(), X.pair_cnt.data()}, K, p->d_xsend[slot].p, p->d_xrecv.p, p->err, reduced);
    if (reduced) { ++p->st_allreduces; p->st_bytes_allreduce += (double)reduced * sizeof(double); }
    if (rc != PGO_OK) return rc;
    unpack(p->d_xrecv.p);
    return PGO_OK;
}

// Multi-GPU exchange of the keyframes' rows: sums, over the ranks sharing them, the rows of one or two keyframe-indexed device arrays (k1 + k2 doubles per keyframe).  Every rank
// sends its partial rows of the keyframes it shares with a peer to that peer and adds what it receives in ascending rank order (pgo_mg_host.hpp: build_fine_plan): all ranks
// end up with the same bits.  Keyframes touched by a single rank never travel.  `stop` (device flag): a stopped PCG sends zeros and keeps its rows.
int exchange_rows(pgo_problem* p, double* a1, int k1, double* a2, int k2, const int32_t* stop) {
    if (!p->local_ids) return PGO_OK;
    const pgo_mg::FinePlan& F = p->fine_plan;
    return neighbor_exchange(p, F.x, k1 + k2, [&](double* sb) { launch_gather_rows(sb, a1, k1, a2, k2, F.x.n_send(), p->d_fp_send.p, stop, p->st); },
                             [&](const double* rb) { launch_sum_rows(rb, a1, k1, a2, k2, (int64_t)F.sh_loc.size(), p->d_fp_shloc.p, p->d_fp_sumptr.p, p->d_fp_sumsrc.p, stop, p->st); });
}
// ... and of the multigrid's level vectors: the rows of one or two vectors of level `l + 1` this rank owns and a peer reads go to that peer, the rows it reads come in
int exchange_level(pgo_problem* p, int l, double* v1, double* v2, const int32_t* stop, const double* dinv) {
    if (!p->local_ids || (size_t)l >= p->mg.lvl_plan.size() || !p->mg.lvl_plan[(size_t)l].plan) return PGO_OK;
    const LevelPlanDev& L = p->mg.lvl_plan[(size_t)l];
    if (dinv)      // x = v1, r = v2: only r travels, x = Dinv r is formed on receipt (pointwise; every rank holds the level's Dinv)
        return neighbor_exchange(p, *L.plan, 6, [&](double* sb) { launch_gather_rows(sb, v2, 6, nullptr, 0, L.plan->n_send(), L.send_idx, stop, p->st); },
                                 [&](const double* rb) { launch_scatter_rows_dinv(rb, v2, v1, dinv, L.plan->n_recv(), L.recv_idx, stop, p->st); });
    return neighbor_exchange(p, *L.plan, v2 ? 12 : 6, [&](double* sb) { launch_gather_rows(sb, v1, 6, v2, v2 ? 6 : 0, L.plan->n_send(), L.send_idx, stop, p->st); },
                             [&](const double* rb) { launch_scatter_rows(rb, v1, 6, v2, v2 ? 6 : 0, L.plan->n_recv(), L.recv_idx, stop, p->st); });
}
// ... and of the multigrid's SET-UP (distributed set-up, round 6): 6x6 blocks listed by slot (K doubles each: 36, or 18 for an fp32 block).  Copy: every block has one producer.
// Sum: the parts of a block formed on several ranks are added, in ascending rank order, on every rank that needs it (pgo_mg_host.hpp: BlockPlan).  A plan with nothing to send
// anywhere (pair_cnt, the same on all ranks) is skipped by all of them.
static bool plan_is_empty(const pgo_mg::ExchangePlan& X) { for (int64_t c : X.pair_cnt) if (c) return false; return true; }
int exchange_blocks_copy(pgo_problem* p, const pgo_mg::ExchangePlan& X, const int32_t* send_idx, const int32_t* recv_idx, double* arr, int K) {
    if (plan_is_empty(X)) return PGO_OK;
    return neighbor_exchange(p, X, K, [&](double* sb) { launch_gather_rows(sb, arr, K, nullptr, 0, X.n_send(), send_idx, nullptr, p->st); },
                             [&](const double* rb) { launch_scatter_rows(rb, arr, K, nullptr, 0, X.n_recv(), recv_idx, nullptr, p->st); });
}
int exchange_blocks_sum(pgo_problem* p, const pgo_mg::BlockPlan& B, const SetupPlanDev& D, double* arr) {
    if (plan_is_empty(B.x)) return PGO_OK;
    return neighbor_exchange(p, B.x, 36, [&](double* sb) { launch_gather_rows(sb, arr, 36, nullptr, 0, B.x.n_send(), D.val_send, nullptr, p->st); },
                             [&](const double* rb) { launch_sum_rows(rb, arr, 36, nullptr, 0, (int64_t)B.dst.size(), D.val_dst, D.val_sum_ptr, D.val_sum_src, nullptr, p->st); });
}
// all-reduce of a host vector (graph build: rare, sizes up to a few tens of MB)
int host_allreduce(pgo_problem* p, std::vector<double>& v, int op) {
    if (v.empty()) return PGO_OK;
    HIPCHK(p, p->d_tmp.ensure(v.size()));
    HIPCHK(p, hipMemcpyAsync(p->d_tmp.p, v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice, p->st));
    int rc;
    if ((rc = allreduce(p, p->d_tmp.p, v.size(), op)) != PGO_OK) return rc;
    HIPCHK(p, hipMemcpyAsync(v.data(), p->d_tmp.p, v.size() * sizeof(double), hipMemcpyDeviceToHost, p->st));
    HIPCHK(p, hipStreamSynchronize(p->st));
    return PGO_OK;
}

}  // namespace pgo

namespace {

// keyframe-indexed device array of this handle (k doubles per keyframe) -> the caller's array over ALL keyframes, complete on every rank
// (multi-GPU: each keyframe is contributed by its owner; keyframes no rank touches come back as zeros)
int nodes_to_global(pgo_problem* p, const double* dev, int k, double* host_global) {
    if (!p->local_ids) {
        HIPCHK(p, hipMemcpyAsync(host_global, dev, (size_t)p->N * k * sizeof(double), hipMemcpyDeviceToHost, p->st));
        HIPCHK(p, hipStreamSynchronize(p->st));
        return PGO_OK;
    }
    std::vector<double> loc((size_t)p->N * k), glob((size_t)p->N_global * k, 0.0);
    HIPCHK(p, hipMemcpyAsync(loc.data(), dev, loc.size() * sizeof(double), hipMemcpyDeviceToHost, p->st));
    HIPCHK(p, hipStreamSynchronize(p->st));
    for (int64_t l = 0; l < p->N; ++l) if (p->h_own[l] != 0.0) std::copy(loc.begin() + l * k, loc.begin() + (l + 1) * k, glob.begin() + (size_t)p->l2g[l] * k);
    HIPCHK(p, p->d_tmp.ensure(glob.size()));
    HIPCHK(p, hipMemcpyAsync(p->d_tmp.p, glob.data(), glob.size() * sizeof(double), hipMemcpyHostToDevice, p->st));
    int rc;
    if ((rc = allreduce(p, p->d_tmp.p, glob.size(), 0)) != PGO_OK) return rc;
    HIPCHK(p, hipMemcpyAsync(host_global, p->d_tmp.p, glob.size() * sizeof(double), hipMemcpyDeviceToHost, p->st));
    HIPCHK(p, hipStreamSynchronize(p->st));
    return PGO_OK;
}
// the caller's array over all keyframes -> this handle's keyframes on the device
int nodes_from_global(pgo_problem* p, const double* host_global, int k, double* dev) {
    if (!p->local_ids) {
        HIPCHK(p, hipMemcpyAsync(dev, host_global, (size_t)p->N * k * sizeof(double), hipMemcpyHostToDevice, p->st));
        HIPCHK(p, hipStreamSynchronize(p->st));
        return PGO_OK;
    }
    std::vector<double> loc((size_t)p->N * k);
    for (int64_t l = 0; l < p->N; ++l) std::copy(host_global + (size_t)p->l2g[l] * k, host_global + (size_t)(p->l2g[l] + 1) * k, loc.begin() + l * k);
    HIPCHK(p, hipMemcpyAsync(dev, loc.data(), loc.size() * sizeof(double), hipMemcpyHostToDevice, p->st));
    HIPCHK(p, hipStreamSynchronize(p->st));
    return PGO_OK;
}

double* part(pgo_problem* p, int k) { return p->d_part.p + (size_t)k * p->n_part; }

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
    p->x_norm = std::sqrt(h[S_XNORM2] + h[S_SW_XNORM2]);
    p->gmax = h[S_GMAX];
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
    p->terminated = true;
    p->sum.termination_type = type;
    std::snprintf(p->sum.message, sizeof(p->sum.message), "%s", msg);
}

int solve_begin(pgo_problem* p, const double* quat, const double* t, const double* sw, int64_t N, int64_t S) {
    if (!quat || !t || N <= 0 || S < 0 || (S > 0 && !sw)) { p->err = "null state array or bad size"; return PGO_ERR_INVALID_ARG; }
    int rc;
    if ((rc = set_device(p)) != PGO_OK) return rc;
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
    p->in_solve = true; p->terminated = false; p->scale_ready = false; p->have_prev_step = false;
    p->st_exchanges = p->st_allreduces = p->st_pcg_iterations = 0; p->st_bytes_neighbour = p->st_bytes_allreduce = 0.0;
    p->pcg.cg_prev_equiv = 0.0; p->pcg.cg_prev_radius = 0.0; p->mg.regroups = 0; p->last_rho = 1.0;
    two_level_solve_begin(p);
    p->radius = p->opt.initial_trust_region_radius; p->decrease_factor = 2.0; p->reuse_diagonal = false; p->iteration = 0; p->invalid = 0;
    p->sum.termination_type = PGO_NO_CONVERGENCE;
    if ((rc = linearize(p, &p->x_cost)) != PGO_OK) return rc;
    p->sum.initial_cost = p->x_cost;
    p->sum.final_cost = p->x_cost;
    if (!std::isfinite(p->x_cost)) { terminate(p, PGO_FAILURE, "initial cost is not finite"); return PGO_OK; }
    pgo_iteration it{};
    it.iteration = 0; it.step_is_valid = 1; it.step_is_successful = 1; it.cost = p->x_cost; it.gradient_max_norm = p->gmax; it.trust_region_radius = p->radius;
    it.seconds = now_s() - p->t_device0;
    log_iter(p, it);
    return PGO_OK;
}

int lm_step(pgo_problem* p, int ignore_termination, int* done) {
    if (!p->in_solve) { p->err = "pgo_lm_step before pgo_solve_begin"; return PGO_ERR_STATE; }
    const pgo_options& o = p->opt;
    int rc;
    if ((rc = set_device(p)) != PGO_OK) return rc;
    if (p->terminated && !ignore_termination) { if (done) *done = 1; return PGO_OK; }
    if (p->sum.termination_type == PGO_FAILURE && p->terminated) { if (done) *done = 1; return PGO_OK; }
    // FinalizeIterationAndCheckIfMinimizerCanContinue
    if (!ignore_termination) {
        if (p->iteration >= o.max_num_iterations) { terminate(p, PGO_NO_CONVERGENCE, "Maximum number of iterations reached."); if (done) *done = 1; return PGO_OK; }
        if (p->gmax <= o.gradient_tolerance) { terminate(p, PGO_CONVERGENCE, "Gradient tolerance reached."); if (done) *done = 1; return PGO_OK; }
        if (p->radius < o.min_trust_region_radius) { terminate(p, PGO_CONVERGENCE, "Minimum trust region radius reached."); if (done) *done = 1; return PGO_OK; }
    }
    const double t0 = now_s();
    ++p->iteration;
    pgo_iteration it{};
    it.iteration = p->iteration; it.trust_region_radius = p->radius;
    if (!p->reuse_diagonal) launch_lm_diag(p->G, p->L, p->Sc, o.min_lm_diagonal, o.max_lm_diagonal, p->st);
    bool ok = true;
    if ((rc = build_system(p, &ok)) != PGO_OK) return rc;
    const double t_built = now_s();
    int why_invalid = ok ? PGO_STEP_ACCEPTED : PGO_STEP_INVALID_FACTORIZATION;      // pgo_iteration.reason of an invalid step
    int precond_used = PGO_PRECOND_BLOCK_JACOBI;
    CgResult cg{0, false, 0.0, false};
    p->pcg.cg_extra = 0;
    const int nxt = p->cur ^ 1;
    double h[S_N] = {0};
    // candidate point x (+) delta, its cost, the model cost change and the step norms -> h[]
    auto evaluate_candidate = [&]() -> int {
        int np = 0, np2 = 0, r2;
        launch_model_change(p->G, p->L, p->Sc, p->C.x, p->d_delta_s.p, part(p, 4), &np, p->st);
        launch_reduce(part(p, 4), np, 0, p->d_scal.p + S_MODEL, p->st);
        launch_plus(p->G, p->d_pose[p->cur].p, p->d_swv[p->cur].p, p->C.x, p->d_delta_s.p, p->d_pose[nxt].p, p->d_swv[nxt].p, part(p, 1), part(p, 2), &np2, p->st);
        launch_reduce(part(p, 1), np2, 0, p->d_scal.p + S_STEP2, p->st);
        launch_reduce(part(p, 2), np2, 0, p->d_scal.p + S_SW_STEP2, p->st);
        if ((r2 = run_k1(p, nxt, false)) != PGO_OK) return r2;
        HIPCHK(p, hipMemsetAsync(p->d_scal.p + S_SW_XNORM2, 0, 2 * sizeof(double), p->st));   // SW_XNORM2, GMAX unused here
        HIPCHK(p, hipMemsetAsync(p->d_scal.p + S_XNORM2, 0, sizeof(double), p->st));
        return read_scalars(p, h);
    };
    bool evaluated = false;
    if (ok) {
        // The PCG pauses at up to two intermediate tolerances (cg_early_tolerance > cg_mid_tolerance > cg_rel_tolerance).  A rejected step
        // only changes the trust-region radius (Ceres StepRejected), so a step that is already clearly bad at a pause
        // (relative_decrease below the stage's threshold, and neither convergence test would fire) is rejected without paying for the
        // remaining decades; otherwise the same PCG resumes towards the next tolerance.
        struct Stage { double tol, reject_rho; };
        Stage stages[2]; int n_stages = 0;
        // A pause costs one candidate evaluation (~0.1 ms: eight small launches and a host sync) and pays only when a step is rejected on a system whose PCG is expensive.  The
        // reference's own sessions (hundreds to a few thousand keyframes, steps accepted almost throughout, PCGs of 20-100 iterations at ~14 us) only pay: measured 20.8 -> 17.1 ms
        // on a 400-keyframe trigger, 63.2 -> 60.3 ms at 3 000.  So below CG_PAUSE_MIN_KEYFRAMES the pauses are armed by the first rejected step of the solve (a rejection is
        // usually followed by more: the radius shrinks in several steps) — a rule that depends on the solve's own history only.
        constexpr int64_t CG_PAUSE_MIN_KEYFRAMES = 20000;
        // ... and (round 5) in proportion to what they can save.  A pause costs ~0.25 ms (candidate evaluation, host round trips, the PCG's restart out of its hipGraph), and a
        // system whose step is ACCEPTED pays it for nothing: 13 of C3's 20 steps, 2.8 % of its headline.
        //   * both pauses where a rejection is in the air — the rule build_system defers the multigrid by: the previous step was rejected (rejections come in streaks) or the last
        //     accepted step's relative decrease fell below 0.8 (C3's and C4's first rejected steps follow rho = 0.67 and 0.62);
        //   * the FIRST pause alone, as cheap insurance, where the system is expensive enough for one wasted solve to outweigh dozens of pauses: predicted block-Jacobi-equivalent
        //     iterations x keyframes >= 5.6e7, i.e. a solve of >= ~20 ms (a pause pair is 0.5 ms; a block-Jacobi iteration costs ~36 us per 100 000 keyframes).  rho does NOT
        //     predict every rejection: C5's step 8 follows rho = 0.97 and is rejected with rho = -2.0 — 1.87 s of PCG thrown away against 0.25 s with the pause
        //     (profiles/r05_pause_rule.txt); a system without a prediction counts as mg_switch_iterations iterations;
        //   * none elsewhere.  The PCG's own iterates do not depend on where it pauses.
        const bool rejection_likely = p->reuse_diagonal || p->last_rho < 0.8;
        const double predicted_its = p->pcg.cg_predicted > 0.0 ? p->pcg.cg_predicted : (double)(o.mg_switch_iterations > 0 ? o.mg_switch_iterations : 400);
        const bool expensive = predicted_its * (double)p->N_global >= 5.6e7;
        const bool armed = p->N_global >= CG_PAUSE_MIN_KEYFRAMES || p->sum.num_unsuccessful_steps > 0;
        const bool pauses = armed && (rejection_likely || p->opt.cg_pause_always != 0);
        const bool early_only = armed && !pauses && expensive;
        if ((pauses || early_only) && o.cg_early_tolerance > o.cg_rel_tolerance) stages[n_stages++] = Stage{o.cg_early_tolerance, o.cg_early_reject_rho};
        if (pauses && o.cg_mid_tolerance > o.cg_rel_tolerance && (n_stages == 0 || o.cg_mid_tolerance < stages[0].tol)) stages[n_stages++] = Stage{o.cg_mid_tolerance, o.cg_mid_reject_rho};
        const bool warm = o.cg_warm_start != 0 && p->have_prev_step && p->reuse_diagonal;
        if ((rc = run_pcg(p, &cg, PcgPhase{n_stages ? stages[0].tol : o.cg_rel_tolerance, -1, warm})) != PGO_OK) return rc;
        for (int sidx = 0; sidx < n_stages && !cg.breakdown && !evaluated; ++sidx) {
            if ((rc = evaluate_candidate()) != PGO_OK) return rc;
            const double mc = -h[S_MODEL];
            const double cand = 0.5 * (h[S_COST] + h[S_PRIOR_COST]);
            const double dc = p->x_cost - cand;
            const double sn = std::sqrt(h[S_STEP2] + h[S_SW_STEP2]);
            const bool clear_reject = mc > 0.0 && std::isfinite(mc) && std::isfinite(cand) && dc / mc < stages[sidx].reject_rho &&
                                      sn > o.parameter_tolerance * (p->x_norm + o.parameter_tolerance) && std::fabs(dc) > o.function_tolerance * p->x_cost;
            if (clear_reject) evaluated = true;
            else {
                const bool to_mg = p->pcg.mg_start_deferred && !p->mg.active;
                p->pcg.mg_start_deferred = false;
                if ((rc = run_pcg(p, &cg, PcgPhase{sidx + 1 < n_stages ? stages[sidx + 1].tol : o.cg_rel_tolerance, cg.iterations, false, to_mg})) != PGO_OK) return rc;
            }
        }
        if ((rc = finish_system(p, &cg, evaluated, &precond_used)) != PGO_OK) return rc;
        p->have_prev_step = !cg.breakdown;
        if (cg.breakdown) { ok = false; why_invalid = PGO_STEP_INVALID_BREAKDOWN; }
    }
    it.cg_iterations = cg.iterations + p->pcg.cg_extra; it.cg_residual = cg.rel_residual;
    const double t_solved = now_s();
    it.seconds_system = t_built - t0; it.seconds_pcg = t_solved - t_built;
    it.cg_iterations_multigrid = p->mg.active ? cg.iterations : 0; it.single_reduction = ok && single_reduction(p) ? 1 : 0;
    if (o.verbosity > 1) std::fprintf(stderr, "[pgo] it %3d PCG: %d iterations%s after %d with block-Jacobi; system + preconditioner %.3f ms, PCG %.3f ms\n", p->iteration, cg.iterations, p->mg.active ? " with the multigrid" : "", p->pcg.cg_extra, (t_built - t0) * 1e3, (t_solved - t_built) * 1e3);
    p->sum.cg_iterations += cg.iterations + p->pcg.cg_extra;
    if (p->mg.active) p->sum.cg_iterations_multigrid += cg.iterations;     // iterations before an in-flight switch (cg_extra) ran with block-Jacobi
    if (ok) {
        if (!evaluated && (rc = evaluate_candidate()) != PGO_OK) return rc;
        it.seconds_evaluate = now_s() - t_solved;
        if (o.verbosity > 1) std::fprintf(stderr, "[pgo] it %3d candidate evaluated in %.3f ms\n", p->iteration, it.seconds_evaluate * 1e3);
        it.model_cost_change = -h[S_MODEL];
        if (!(it.model_cost_change > 0.0) || !std::isfinite(it.model_cost_change)) { ok = false; why_invalid = PGO_STEP_INVALID_MODEL; }
    }
    it.preconditioner = precond_used;
    if (!ok) {
        // HandleInvalidStep
        it.step_is_valid = 0; it.cost = p->x_cost; it.gradient_max_norm = p->gmax; it.reason = why_invalid;
        ++p->invalid; ++p->sum.num_unsuccessful_steps;
        if (p->invalid >= o.max_num_consecutive_invalid_steps && !ignore_termination) {
            terminate(p, PGO_FAILURE, "Number of consecutive invalid steps more than max_num_consecutive_invalid_steps.");
            it.seconds = now_s() - t0; log_iter(p, it);
            if (done) *done = 1;
            return PGO_OK;
        }
        p->radius *= 0.5; p->reuse_diagonal = true;   // LevenbergMarquardtStrategy::StepIsInvalid
        it.seconds = now_s() - t0; log_iter(p, it);
        if (done) *done = 0;
        return PGO_OK;
    }
    p->invalid = 0;
    it.step_is_valid = 1;
    const double cand_cost = 0.5 * (h[S_COST] + h[S_PRIOR_COST]);
    it.step_norm = std::sqrt(h[S_STEP2] + h[S_SW_STEP2]);
    it.cost_change = p->x_cost - cand_cost;
    it.relative_decrease = it.cost_change / it.model_cost_change;
    bool stop = false;
    if (!ignore_termination) {
        if (it.step_norm <= o.parameter_tolerance * (p->x_norm + o.parameter_tolerance)) { terminate(p, PGO_CONVERGENCE, "Parameter tolerance reached."); stop = true; }
        else if (std::fabs(it.cost_change) <= o.function_tolerance * p->x_cost) { terminate(p, PGO_CONVERGENCE, "Function tolerance reached."); stop = true; }
    }
    if (stop) {
        it.reason = PGO_STEP_CONVERGED;
        it.cost = p->x_cost; it.gradient_max_norm = p->gmax; it.seconds = now_s() - t0; log_iter(p, it);
        if (done) *done = 1;
        return PGO_OK;
    }
    if (std::isfinite(cand_cost) && it.relative_decrease > o.min_relative_decrease) {
        // HandleSuccessfulStep
        p->cur = nxt;
        double c = 0;
        const double t_lin = now_s();
        if ((rc = linearize(p, &c)) != PGO_OK) return rc;
        it.seconds_linearize = now_s() - t_lin;
        if (o.verbosity > 1) std::fprintf(stderr, "[pgo] it %3d linearised in %.3f ms\n", p->iteration, it.seconds_linearize * 1e3);
        p->x_cost = c;
        it.step_is_successful = 1;
        p->radius = p->radius / std::max(1.0 / 3.0, 1.0 - std::pow(2.0 * it.relative_decrease - 1.0, 3));   // StepAccepted
        p->radius = std::min(o.max_trust_region_radius, p->radius);
        p->decrease_factor = 2.0; p->reuse_diagonal = false;
        p->last_rho = it.relative_decrease;
        it.reason = PGO_STEP_ACCEPTED;
        ++p->sum.num_successful_steps;
        if ((rc = regroup_start(p)) != PGO_OK) return rc;     // the switches have moved: does the hierarchy above level 1 still fit them?
    } else {
        p->radius = p->radius / p->decrease_factor; p->decrease_factor *= 2.0; p->reuse_diagonal = true;   // StepRejected
        it.reason = evaluated ? PGO_STEP_REJECTED_AT_PAUSE : PGO_STEP_REJECTED_RHO;
        ++p->sum.num_unsuccessful_steps;
    }
    it.cost = p->x_cost; it.gradient_max_norm = p->gmax; it.seconds = now_s() - t0;
    log_iter(p, it);
    p->sum.final_cost = p->x_cost;
    if (done) *done = 0;
    return PGO_OK;
}

int solve_end(pgo_problem* p, double* quat, double* t, double* sw, pgo_summary* out) {
    if (!p->in_solve) { p->err = "pgo_solve_end before pgo_solve_begin"; return PGO_ERR_STATE; }
    int rc;
    if ((rc = set_device(p)) != PGO_OK) return rc;
    const double t_dev = now_s();
    p->sum.num_iterations = p->iteration;
    p->sum.final_cost = p->x_cost;
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
    two_level_solve_end(p);
    if (p->mg.job.kind == MgJob::regroup) mg_drop_pending(p);      // a regroup nobody needed any more: dropped (the hierarchy in place keeps its own switch record)
    if ((rc = mg_fresh_install(p)) != PGO_OK) return rc;      // a fresh graph's hierarchy that this solve never needed: installed now, for the handle's next solves
    p->sum.seconds_total = now_s() - p->t_begin;
    if (out) *out = p->sum;
    p->in_solve = false;
    return PGO_OK;
}

int add_edges(pgo_problem* p, HostClass& H, int64_t n, const int32_t* c1, const int32_t* c2, const double* T, const double* w, const int32_t* sw) {
    if (n < 0 || (n > 0 && (!c1 || !c2 || !T))) { p->err = "null edge array"; return PGO_ERR_INVALID_ARG; }
    for (int64_t k = 0; k < n; ++k) if (c1[k] < 0 || c2[k] < 0 || c1[k] == c2[k] || (sw && sw[k] < 0)) { p->err = "negative index or self edge"; return PGO_ERR_INVALID_ARG; }
    mg_drop_pending(p);      // (the worker reads the edge lists)
    const size_t base = H.c1.size();
    H.c1.insert(H.c1.end(), c1, c1 + n);
    H.c2.insert(H.c2.end(), c2, c2 + n);
    if (sw) H.sw.insert(H.sw.end(), sw, sw + n);
    H.meas.resize((base + n) * 8);
    for (int64_t k = 0; k < n; ++k) meas_from_matrix(T + 16 * k, w ? w[k] : 1.0, &H.meas[(base + k) * 8]);
    p->graph_dirty = true;
    return PGO_OK;
}

// Every pgo_comm_init*: one transport per handle; a new one changes the keyframes this handle works on (the union over ranks), so what was built for the old graph goes
template <class Make>
int attach_comm(pgo_problem* p, Make make) {
    if (p->comm) { p->err = "a communicator is attached: call pgo_comm_destroy first"; return PGO_ERR_INVALID_ARG; }
    int rc;
    std::unique_ptr<pgo_comm::Comm> c;
    if ((rc = set_device(p)) != PGO_OK || (rc = make(c)) != PGO_OK) return rc;
    mg_drop_pending(p);
    p->comm = std::move(c);
    p->graph_dirty = true;
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
int pgo_add_switchable_edges(pgo_problem* p, int64_t n, const int32_t* c1, const int32_t* c2, const double* T, const double* w, const int32_t* sw) {
    if (!p) return PGO_ERR_INVALID_ARG;
    if (n > 0 && !sw) { p->err = "switch index array required"; return PGO_ERR_INVALID_ARG; }
    return add_edges(p, p->swe, n, c1, c2, T, w, sw);
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
    int done = p->terminated ? 1 : 0;
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
    if (cost) *cost = p->x_cost;
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
    const pgo_options& o = p->opt;
    if (!p->reuse_diagonal) launch_lm_diag(p->G, p->L, p->Sc, o.min_lm_diagonal, o.max_lm_diagonal, p->st);
    bool ok = true;
    if ((rc = build_system(p, &ok)) != PGO_OK) return rc;
    // x and y are arrays over ALL keyframes (multi-GPU: this rank applies its part to its keyframes, shared rows are summed)
    HIPCHK(p, p->d_io.ensure((size_t)p->N * 12));
    double* xin = p->d_io.p; double* yout = p->d_io.p + (size_t)p->N * 6;
    if ((rc = nodes_from_global(p, x, 6, xin)) != PGO_OK) return rc;
    if (p->built_mf) launch_mf_apply(p->G, p->F, p->Sc, p->C, xin, yout, p->st);
    else launch_apply_operator(p->G, p->C, xin, yout, p->st);
    if ((rc = exchange_rows(p, yout, 6, nullptr, 0)) != PGO_OK) return rc;
    return nodes_to_global(p, yout, 6, y);
}

// ---- multi-GPU ----
int pgo_comm_init(pgo_problem* p, int32_t rank, int32_t world, const uint8_t id[PGO_COMM_ID_BYTES]) {
    if (!p || !id || world < 1 || rank < 0 || rank >= world) return PGO_ERR_INVALID_ARG;
    return attach_comm(p, [&](std::unique_ptr<pgo_comm::Comm>& c) { return pgo_comm::make_rccl_comm(id, rank, world, p->st, c, p->err); });
}
int pgo_comm_init_custom(pgo_problem* p, int32_t rank, int32_t world, pgo_allreduce_fn fn, void* ctx) {
    if (!p || !fn || world < 1 || rank < 0 || rank >= world) return PGO_ERR_INVALID_ARG;
    return attach_comm(p, [&](std::unique_ptr<pgo_comm::Comm>& c) { c = pgo_comm::make_custom_comm(fn, ctx, rank, world, p->st); return PGO_OK; });
}
int pgo_comm_set_exchange(pgo_problem* p, pgo_exchange_fn fn) {
    return p && p->comm && p->comm->set_exchange(fn) ? PGO_OK : PGO_ERR_INVALID_ARG;      // (belongs to a communicator set up by pgo_comm_init_custom)
}
int pgo_comm_init_local(pgo_problem* p, int32_t rank, int32_t world, void* group) {
    if (!p || !group || rank < 0 || rank >= world) return PGO_ERR_INVALID_ARG;
    return attach_comm(p, [&](std::unique_ptr<pgo_comm::Comm>& c) { return pgo_comm::make_local_comm(group, rank, world, p->device, p->st, c, p->err); });
}
int pgo_get_sharding_stats(pgo_problem* p, pgo_sharding_stats* out) {
    if (!p || !out) return PGO_ERR_INVALID_ARG;
    std::memset(out, 0, sizeof(*out));
    out->world = p->world(); out->rank = p->rank();
    if (!p->local_ids || p->graph_dirty) return PGO_OK;
    out->keyframes_local = p->N;
    for (double w : p->h_own) if (w != 0.0) ++out->keyframes_owned;
    out->keyframes_shared = p->n_sh_mine; out->shared_global = p->n_sh_global;
    out->pcg_iterations = p->st_pcg_iterations; out->exchanges = p->st_exchanges; out->allreduces = p->st_allreduces;
    out->bytes_sent_neighbour = p->st_bytes_neighbour; out->bytes_allreduce = p->st_bytes_allreduce;
    const double fine = (double)p->fine_plan.x.n_send() * 48.0 + 16.0;
    out->bytes_sent_per_bj_iteration = fine; out->exchanges_per_bj_iteration = 1;
    out->bytes_round5_per_bj_iteration = (6.0 * (double)p->n_sh_global + 2.0) * 8.0;
    if (p->mg.built && !p->mg.fresh_pending() && p->mg.M.n_levels >= 1) {
        const int nl = p->mg.M.n_levels;
        out->mg_levels = nl; out->mg_levels_distributed = p->mg.levels_distributed;
        out->mg_rows_total = p->mg.rows_total; out->mg_rows_own = p->mg.rows_own; out->mg_blocks_total = p->mg.blocks_total; out->mg_blocks_own = p->mg.blocks_own;
        double bytes = fine; int nx = 1;
        auto count = [&](int point, int lv) { int plan; double* v1; double* v2; const double* dinv; if (mg_exchange_at(p, point, lv, &plan, &v1, &v2, &dinv) && p->mg.lvl_plan[(size_t)plan].plan) { bytes += (double)p->mg.lvl_plan[(size_t)plan].plan->n_send() * (v2 && !dinv ? 96.0 : 48.0); ++nx; } };
        for (int l = 1; l <= nl; ++l) count(0, l);
        for (int l = nl - 1; l >= 1; --l) count(1, l);
        count(2, 1);
        out->bytes_sent_per_mg_iteration = bytes; out->exchanges_per_mg_iteration = nx;
        out->bytes_round5_per_mg_iteration = (6.0 * (double)p->n_sh_global + 2.0 + 6.0 * (double)p->mg.M.n1) * 8.0;
        // the set-up: blocks formed per LM system (level matrices; Ps, W and R^T of smoothed transitions), by all and by this rank; what its exchanges send
        const int fw = p->mg.first_whole;
        for (int l = 0; l + 1 < nl; ++l) {
            const MgLevelDev& A = p->mg.levels[l];
            const int64_t all = A.nnzb + (A.smoothed ? (int64_t)A.n_ps + 2 * (int64_t)A.n_w : 0);
            const int64_t own = l < fw ? (A.su_blk1 - A.su_blk0) + (A.smoothed ? (int64_t)(A.su_ps1 - A.su_ps0) + 2 * (int64_t)(A.su_w1 - A.su_w0) : 0) : all;
            out->mg_setup_blocks_total += all; out->mg_setup_blocks_own += own;
        }
        out->bytes_allreduce_replicated_setup = (double)p->mg.levels[0].nnzb * 288.0;
        out->mg_setup_levels_own_rows = fw; out->mg_setup_exchanges = 1;
        if (fw > 0) {
            double sb = 0.0; int nx = 0;
            auto add = [&](const pgo_mg::ExchangePlan& X, double bytes_per_row) { if (!plan_is_empty(X)) { sb += (double)X.n_send() * bytes_per_row; ++nx; } };
            for (const pgo_mg::BlockPlan& B : p->mg.setup.val) add(B.x, 288.0);
            for (int l = 0; l < fw; ++l) {
                nx += 9; sb += 24.0;      // the level's power method: eight halo exchanges of the iterate + the 3-double all-reduce
                if ((size_t)l < p->mg.lvl_plan.size() && p->mg.lvl_plan[(size_t)l].plan) sb += 8.0 * (double)p->mg.lvl_plan[(size_t)l].plan->n_send() * 48.0;
                if (!p->mg.levels[l].smoothed) continue;
                if ((size_t)l < p->mg.lvl_plan.size() && p->mg.lvl_plan[(size_t)l].plan) add(*p->mg.lvl_plan[(size_t)l].plan, 288.0);
                add(p->mg.setup.ps[(size_t)l], 288.0); add(p->mg.setup.rv[(size_t)l], 144.0);
            }
            out->bytes_sent_per_mg_setup = sb; out->mg_setup_exchanges = nx;
        }
    }
    return PGO_OK;
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
int pgo_comm_destroy(pgo_problem* p) {
    if (!p) return PGO_ERR_INVALID_ARG;
    p->comm.reset();
    mg_drop_pending(p);
    p->graph_dirty = true;
    return PGO_OK;
}

// ---- edge sharding policies (host only) ----
int pgo_partition_edges(int32_t policy, int32_t world, int64_t n_nodes, const double* t_xyz, int64_t n_rel, const int32_t* rel_c1, const int32_t* rel_c2,
                        int64_t n_sw, const int32_t* sw_c1, const int32_t* sw_c2, int32_t* node_part, int32_t* rel_rank, int32_t* sw_rank) {
    if (world < 1 || n_nodes < 0 || n_rel < 0 || n_sw < 0 || (n_rel > 0 && (!rel_c1 || !rel_c2 || !rel_rank)) || (n_sw > 0 && (!sw_c1 || !sw_c2 || !sw_rank))) return PGO_ERR_INVALID_ARG;
    if (policy == PGO_PARTITION_CONTIGUOUS) {
        // rank r holds the edges [n r / world, n (r+1) / world) of each class
        for (int cls = 0; cls < 2; ++cls) {
            const int64_t n = cls ? n_sw : n_rel; int32_t* out = cls ? sw_rank : rel_rank;
            for (int r = 0; r < world; ++r) for (int64_t e = (n * r) / world; e < (n * (r + 1)) / world; ++e) out[e] = r;
        }
        return PGO_OK;
    }
    if (policy != PGO_PARTITION_CHAIN && policy != PGO_PARTITION_SPATIAL) return PGO_ERR_INVALID_ARG;
    if (policy == PGO_PARTITION_SPATIAL && n_nodes > 0 && !t_xyz) return PGO_ERR_INVALID_ARG;
    for (int64_t e = 0; e < n_rel; ++e) if (rel_c1[e] < 0 || rel_c1[e] >= n_nodes || rel_c2[e] < 0 || rel_c2[e] >= n_nodes) return PGO_ERR_INVALID_ARG;
    for (int64_t e = 0; e < n_sw; ++e) if (sw_c1[e] < 0 || sw_c1[e] >= n_nodes || sw_c2[e] < 0 || sw_c2[e] >= n_nodes) return PGO_ERR_INVALID_ARG;
    // parts are balanced by the edges they will receive (an edge goes with its later endpoint); keyframes without edges still spread evenly
    std::vector<double> load((size_t)n_nodes, 0.0);
    for (int64_t e = 0; e < n_rel; ++e) load[std::max(rel_c1[e], rel_c2[e])] += 1.0;
    for (int64_t e = 0; e < n_sw; ++e) load[std::max(sw_c1[e], sw_c2[e])] += 1.0;
    for (double& v : load) v += 1e-3;
    std::vector<int32_t> part((size_t)n_nodes, 0);
    if (policy == PGO_PARTITION_CHAIN) {
        std::vector<double> c((size_t)n_nodes);
        double acc = 0.0;
        for (int64_t i = 0; i < n_nodes; ++i) { acc += load[i]; c[i] = acc; }
        for (int64_t i = 0; i < n_nodes; ++i) part[i] = (int32_t)std::min((c[i] - load[i]) * (double)world / acc, (double)(world - 1));
    } else {
        // recursive coordinate bisection: cells [lo, hi) get the keyframes idx[b, e); split along the axis of largest extent at the load quantile
        std::vector<int32_t> idx((size_t)n_nodes), tmp;
        for (int64_t i = 0; i < n_nodes; ++i) idx[i] = (int32_t)i;
        struct Job { int64_t b, e; int lo, hi; };
        std::vector<Job> stack{{0, n_nodes, 0, world}};
        while (!stack.empty()) {
            const Job j = stack.back(); stack.pop_back();
            if (j.hi - j.lo <= 1 || j.e - j.b <= 0) { for (int64_t k = j.b; k < j.e; ++k) part[idx[k]] = j.lo; continue; }
            const int mid = (j.lo + j.hi) / 2;
            double mn[3] = {1e300, 1e300, 1e300}, mx[3] = {-1e300, -1e300, -1e300};
            for (int64_t k = j.b; k < j.e; ++k) for (int a = 0; a < 3; ++a) { const double v = t_xyz[(size_t)idx[k] * 3 + a]; mn[a] = std::min(mn[a], v); mx[a] = std::max(mx[a], v); }
            int axis = 0;
            for (int a = 1; a < 3; ++a) if (mx[a] - mn[a] > mx[axis] - mn[axis]) axis = a;
            std::stable_sort(idx.begin() + j.b, idx.begin() + j.e, [&](int32_t x, int32_t y) { return t_xyz[(size_t)x * 3 + axis] < t_xyz[(size_t)y * 3 + axis]; });
            const int64_t len = j.e - j.b;
            std::vector<double> c((size_t)len);
            double acc = 0.0;
            for (int64_t k = 0; k < len; ++k) { acc += load[idx[j.b + k]]; c[k] = acc; }
            const double target = acc * (double)(mid - j.lo) / (double)(j.hi - j.lo);
            int64_t k = std::lower_bound(c.begin(), c.end(), target) - c.begin();
            if (len > 1) k = std::min(std::max<int64_t>(k, 1), len - 1); else k = len;
            stack.push_back({j.b + k, j.e, mid, j.hi});
            stack.push_back({j.b, j.b + k, j.lo, mid});
        }
    }
    for (int64_t e = 0; e < n_rel; ++e) rel_rank[e] = part[std::max(rel_c1[e], rel_c2[e])];
    for (int64_t e = 0; e < n_sw; ++e) sw_rank[e] = part[std::max(sw_c1[e], sw_c2[e])];
    if (node_part) std::copy(part.begin(), part.end(), node_part);
    return PGO_OK;
}

// ---- measurement helpers ----
int pgo_time_kernel(pgo_problem* p, int32_t which, int32_t launches, double* avg_ms, double* algorithmic_bytes) {
    if (!p || launches <= 0 || !avg_ms) return PGO_ERR_INVALID_ARG;
    if (!p->in_solve) { p->err = "pgo_time_kernel needs an open solve (pgo_solve_begin)"; return PGO_ERR_STATE; }
    int rc;
    if ((rc = set_device(p)) != PGO_OK) return rc;
    EventPair ev;
    HIPCHK(p, ev.create());
    const hipEvent_t e0 = ev.e0, e1 = ev.e1;
    int np = 0;
    const int nxt = p->cur ^ 1;
    const GraphDev& G = p->G;
    double bytes = 0, best_ms = -1.0;
    if (which == 6 || which == 7 || which == 8) {   // one multigrid-preconditioned PCG iteration (6) / its level kernels alone (7) / the kernels of the multigrid's set-up (8), on the current LM system
        if (!p->mg.built || !p->built_mf || (p->local_ids && which == 6)) { p->err = "pgo_time_kernel: this graph has no multigrid hierarchy (mg_min_keyframes) / several ranks: only the level kernels (7) can be timed"; return PGO_ERR_STATE; }
        const pgo_options& o = p->opt;
        if (!p->reuse_diagonal) launch_lm_diag(p->G, p->L, p->Sc, o.min_lm_diagonal, o.max_lm_diagonal, p->st);
        bool ok = true;
        if ((rc = build_system(p, &ok)) != PGO_OK) return rc;
        if (!p->mg.active && (rc = build_mg(p)) != PGO_OK) return rc;
        if (!p->mg.active) { p->err = "pgo_time_kernel: the multigrid operators of this system are not positive definite"; return PGO_ERR_NUMERIC; }
        if (!p->local_ids) { if ((rc = pcg_start(p, choose_form(p), false, 0.0)) != PGO_OK) return rc; }      // (tolerance 0: never converges during the timed launches)
        else { launch_cg_init_vectors(p->G, p->C, 0, p->st); if ((rc = mg_apply_ranks(p, false)) != PGO_OK) return rc; launch_cg_set_tolerance(p->C, 0.0, p->st); }      // (one full distributed cycle: every level vector holds finite numbers)
    }
    // several ranks: the timed launches take turns (every rank's figure is what its GPU would need on its own); only the in-process ranks, which share the GPU(s), wait for each other
    const int turns = (p->comm && (which == 7 || which == 8)) ? p->world() : 1;
    for (int turn = 0; turn < turns; ++turn) {
    if (turns > 1) { HIPCHK(p, hipStreamSynchronize(p->st)); if (!p->comm->barrier()) { p->err = "in-process communicator: a rank left during pgo_time_kernel"; return PGO_ERR_COMM; } if (turn != p->rank()) continue; }
    if (which == 5 && single_reduction(p)) {      // (its head needs the u.w partials of a matvec on the CURRENT u: launched back to back it sees stale ones, breaks down and returns early)
        p->err = "pgo_time_kernel(5): the single-reduction update cannot be timed without its matvec; time the iteration (2) and the matvec (4) and subtract"; return PGO_ERR_STATE;
    }
    if (which == 2 || which == 4 || which == 5) {   // a live PCG state to iterate on (tolerance 0: never converges during the timed launches)
        const pgo_options& o = p->opt;
        if (!p->reuse_diagonal) launch_lm_diag(p->G, p->L, p->Sc, o.min_lm_diagonal, o.max_lm_diagonal, p->st);
        bool ok = true;
        if ((rc = build_system(p, &ok)) != PGO_OK) return rc;
        p->mg.active = false; p->coarse.active = false; p->C.extra_rz = 0;   // the timed iteration is the plain block-Jacobi one: no partial-sum slots of a multigrid / two-level solve
        launch_cg_init(p->G, p->C, 0, 0.0, p->st);
    }
    const double N = (double)G.N, E = (double)(G.rel.E + G.sw.E), Es = (double)G.sw.E;
    // one untimed launch first (instruction cache, TLB).  In-process ranks: three timed batches, the fastest counts — the first batch after a solve_begin that regrouped the
    // hierarchy was measured at 3-5x the steady figure on every rank (C5 on 8 ranks: 0.47-0.82 ms, then 0.146-0.168 ms call after call): eight handles' old images going back to
    // the system stall the GPU's address translation for tens of milliseconds
    const int batches = turns > 1 ? 3 : 1;
    for (int rep = 0; rep < 1 + batches; ++rep) {
        const int n = rep == 0 ? 1 : launches;
        if (rep >= 1) HIPCHK(p, hipEventRecord(e0, p->st));
        for (int i = 0; i < n; ++i) {
            switch (which) {
                case 0: launch_k1(G, p->d_pose[p->cur].p, p->d_swv[p->cur].p, true, part(p, 0), &np, p->st); bytes = k1_algorithmic_bytes(G, true); break;
                case 1: launch_k2(G, p->L, !p->built_mf, p->st, p->built_mf ? &p->F : nullptr); bytes = (624.0 * G.rel.E + 688.0 * Es) + 288.0 * E + 336.0 * N + 112.0 * Es; break;
                case 2: case 4: case 5: {   // one PCG iteration (2), its matvec alone (4), its vector update alone (5)
                          const int kk = rep == 0 ? 0 : i + 1;
                          const PcgForm f = choose_form(p, true);      // the form the solver runs on this handle (several ranks: the rank's own iteration, no exchanges)
                          const bool sr = f.single_red();
                          if (which != 5) pcg_matvec(p, f, kk, 0.0);
                          if (which != 4 && (rc = pcg_update(p, f, kk)) != PGO_OK) return rc;
                          // Bytes this design moves per iteration, each array once.  Matrix-free matvec: per LANE (a relative-pose edge with both
                          // keyframes in one tile is one lane, every other edge side its own) the compact record (8 double2 planes; 11 for switchable
                          // sides) + 12 B of index data (+ a_inv for switchable sides); per keyframe z and p_prev read, p and q written (4 x 48),
                          // damping 48, side ranges / regulariser index / free flag 13.  Update: r, q, p, x read, r, x, z written (7 x 48), the fp32
                          // block-Jacobi factor 96.  Block-CSR matvec: SURVEY.md 8d's assembled form.
                          const double lanes_rel = (double)(p->mf_pair_lanes + p->mf_rel_side_lanes), lanes_sw = (double)p->mf_sw_lanes;
                          // Single-reduction form: the matvec reads u and writes w (2 x 48 per keyframe instead of 4 x 48); the update reads u, w, p, s, x, r and writes p, s, x, r, u (11 x 48).
                          const double mv = p->built_mf ? lanes_rel * (128.0 + 12.0) + lanes_sw * (128.0 + 12.0 + 8.0) + N * ((sr ? 2.0 : 4.0) * 48.0 + 48.0 + 13.0)
                                                        : 288.0 * (N + 2.0 * E) + 4.0 * (N + 2.0 * E) + N * 4.0 * 48.0;
                          const double up = N * ((sr ? 11.0 : 7.0) * 48.0 + 96.0);
                          bytes = which == 2 ? mv + up : which == 4 ? mv : up;
                          break; }
                case 3: launch_k1(G, p->d_pose[nxt].p, p->d_swv[nxt].p, false, part(p, 5), &np, p->st); bytes = k1_algorithmic_bytes(G, false); break;
                case 6: case 7: {
                          const int kk = rep == 0 ? 0 : i + 1;
                          if (p->local_ids) {      // several ranks (7 only): this rank's share of the cycle's kernels, no exchanges (what its GPU computes per cycle)
                              launch_mg_apply(G, p->C, p->mg.M, p->mg.levels, p->coarse.K, p->C.r, p->C.z, p->C.part_rz, mg_scale(p), false, p->st, false, mg_cs(p), nullptr);
                              bytes = (double)p->mg.blocks_own * 148.0 + (double)p->mg.rows_own * (288.0 + 24.0 + 8.0 * 48.0 + 16.0) + (double)p->coarse.K.nc * (double)p->coarse.K.nc * 4.0 + (double)p->coarse.K.nc * 16.0;
                              break;
                          }
                          PcgForm f = choose_form(p);
                          const bool sr = f.single_red();
                          if (which == 6) { pcg_matvec(p, f, kk, 0.0); if ((rc = pcg_update(p, f, kk)) != PGO_OK) return rc; }
                          else { f.post = PcgForm::mg_cycle; f.split = UpdSplit{}; }      // (the cycle alone: the restriction is its own, no update in front and no riders)
                          if ((rc = pcg_precond(p, f, kk)) != PGO_OK) return rc;
                          // Bytes of this design, each array once per kernel that streams it.  Fine level as in case 2 (+ the restriction's per-keyframe offsets and slot table,
                          // the prolongation's read-modify-write of z, offsets and aggregate index); every sparse coarse level: its fp32 blocks and column indices twice
                          // (down- and up-sweep), Dinv, positions/offsets and its four vectors; the dense level: the fp32 inverse once.
                          const double lanes_rel = (double)(p->mf_pair_lanes + p->mf_rel_side_lanes), lanes_sw = (double)p->mf_sw_lanes;
                          const double fine = lanes_rel * (128.0 + 12.0) + lanes_sw * (128.0 + 12.0 + 8.0) + N * ((sr ? 2.0 : 4.0) * 48.0 + 48.0 + 13.0) + N * ((sr ? 11.0 : 7.0) * 48.0 + 96.0);
                          double cyc = N * (24.0 + 16.0 / 8.0 * 8.0) /* d0 + slot table (restriction) */ + N * (2.0 * 48.0 + 24.0 + 4.0 + 4.0) /* z read + write, d0, agg0, member list (prolongation) */;
                          for (int l = 0; l + 1 < p->mg.M.n_levels; ++l) {
                              const MgLevelDev& A = p->mg.levels[l];
                              if (A.smoothed && A.rt_valf)      // explicit transfer operator: the level's own blocks once (smoothing step), R and R^T once each, Dinv once, r / x / y / xf and the level above's r, x
                                  cyc += (double)A.nnzb * (144.0 + 4.0) + 2.0 * (double)A.n_w * (144.0 + 4.0) + (double)A.n * (288.0 + 24.0 + 8.0 * 48.0 + 16.0) + (double)A.n_next * (288.0 + 2.0 * 48.0 + 8.0);
                              else
                              cyc += (A.smoothed ? 4.0 : 2.0) * (double)A.nnzb * (144.0 + 4.0) + (double)A.n * ((A.smoothed ? 4.0 : 2.0) * 288.0 /* Dinv: smoothing steps */ + 24.0 + (A.smoothed ? 18.0 : 10.0) * 48.0 + 16.0);
                          }
                          cyc += (double)p->coarse.K.nc * (double)p->coarse.K.nc * 4.0 + (double)p->coarse.K.nc * 16.0;
                          if (f.split.on()) cyc += N * 48.0;      // the split update: the block-Jacobi rider reads the new residual back
                          bytes = which == 6 ? fine + cyc : cyc;
                          break; }
                case 8: {     // this rank's kernels of one multigrid set-up (operators of an LM system incl. the dense inverse), without the exchanges between them
                          const bool hoff_valid = !p->built_mf || p->hoff_epoch == p->lin_epoch;
                          if ((rc = mg_operators(p, p->coarse.d_cinfo.p, hoff_valid, true, -1.0)) != PGO_OK) return rc;
                          bytes = 0.0;
                          break; }
                default: return PGO_ERR_INVALID_ARG;
            }
        }
        if (rep >= 1) HIPCHK(p, hipEventRecord(e1, p->st));
        HIPCHK(p, hipStreamSynchronize(p->st));
        if (rep >= 1) { float msb = 0; HIPCHK(p, hipEventElapsedTime(&msb, e0, e1)); if (best_ms < 0.0 || (double)msb < best_ms) best_ms = (double)msb; }
    }
    }
    if (turns > 1 && !p->comm->barrier()) { p->err = "in-process communicator: a rank left during pgo_time_kernel"; return PGO_ERR_COMM; }
    if (which == 8) { p->mg.active = false; if ((rc = build_mg(p)) != PGO_OK) return rc; }      // (several ranks: the timed kernels ran without their exchanges — the operators are formed again, properly)
    *avg_ms = best_ms / launches;
    if (algorithmic_bytes) *algorithmic_bytes = bytes;
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
