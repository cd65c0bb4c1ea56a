// pgo_shard.hip — everything multi-rank above the transport (pgo_comm.hip): the rank-local subgraph of a graph build, the collectives and neighbour exchanges of the solve
// and of the multigrid's set-up, keyframe arrays between the rank's numbering and the caller's, the communicator entry points of the C-ABI, the sharding counters and the
// edge sharding policies.  On one GPU, without a communicator, the collectives and exchanges are no-ops.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "pgo_handle.hpp"

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

// Graph build, several ranks: the rank-local subgraph.  This rank works on the keyframes its own residual blocks touch, renumbered densely (p->l2g, p->g2l, *n_local of them);
// keyframes touched by >= 2 ranks are "shared" (their rows are summed over ranks by exchange_rows), one touching rank is the owner (p->h_owner, p->h_own; G.own on the device).
// Also the keyframes' exchange plan and the exchange buffers.  Two collectives, on every rank: a sum all-reduce, then a max all-reduce.  One GPU: nothing to number.
int number_rank_local(pgo_problem* p, int64_t Ng, int64_t* n_local) {
    p->local_ids = p->comm != nullptr;   // also with a 1-rank communicator: the same code path, every collective issued
    p->n_sh_mine = p->n_sh_global = 0;
    if (!p->local_ids) {
        p->l2g.clear(); p->g2l.clear(); p->h_own.clear(); p->h_touched_any.clear();
        p->G.own = nullptr;
        *n_local = Ng;
        return PGO_OK;
    }
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
    int rc;
    if ((rc = host_allreduce(p, buf, 0)) != PGO_OK) return rc;
    if ((rc = host_allreduce(p, obuf, 2)) != PGO_OK) return rc;
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
    HIPCHK(p, p->d_l2g.upload(p->l2g, p->st)); HIPCHK(p, p->d_own.upload(p->h_own, p->st));
    // the keyframes' neighbour exchange: segments per peer, and for every shared keyframe the order its parts are summed in (pgo_mg_host.hpp: build_fine_plan)
    pgo_mg::build_fine_plan(p->h_touch_mask, p->l2g, p->rank(), p->world(), p->fine_plan);
    const pgo_mg::FinePlan& F = p->fine_plan;
    HIPCHK(p, p->d_fp_send.upload(F.x.send_idx, p->st)); HIPCHK(p, p->d_fp_shloc.upload(F.sh_loc, p->st));
    HIPCHK(p, p->d_fp_sumptr.upload(F.sum_ptr, p->st)); HIPCHK(p, p->d_fp_sumsrc.upload(F.sum_src, p->st));
    p->mg.lvl_plan.clear();
    if ((rc = ensure_exchange_buffers(p)) != PGO_OK) return rc;
    HIPCHK(p, hipStreamSynchronize(p->st));
    p->G.own = p->d_own.p;
    *n_local = (int64_t)p->l2g.size();
    return PGO_OK;
}

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

}  // namespace pgo

namespace {

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

extern "C" {

// ---- the handle's communicator, its sharding counters ----
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
int pgo_comm_destroy(pgo_problem* p) {
    if (!p) return PGO_ERR_INVALID_ARG;
    p->comm.reset();
    mg_drop_pending(p);
    p->graph_dirty = true;
    return PGO_OK;
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

}  // extern "C"
