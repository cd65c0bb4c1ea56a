// pgo_multigrid.hip — host lifecycle of the aggregation multigrid preconditioner: the hierarchy's host half (pgo_mg_host.hpp + the pooled arrays and device descriptors of its
// image), its install, the one host build that may be in flight (a fresh graph's hierarchy or a regroup), the operators of each LM system and the several-rank cycle's exchanges.
// The kernels are pgo_mg_kernels.hpp's; the handle is pgo_handle.hpp's, the collectives pgo_shard.hip's, the two-level method pgo_pcg.hip's.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <thread>
#include <vector>

#include "pgo_handle.hpp"

namespace pgo {

// Host half of a multigrid build: the hierarchy, the three pools of its device image and the device descriptors that point into them.  No HIP call, no collective in here
// when the handle is a single rank's — that half can therefore run on a worker thread while the stream works on other LM steps; mg_install() uploads it.
// Every descriptor pointer is recorded where its array is appended to a pool (a relocation: field, pool, element offset) and set by mg_install once the pools are on the device.
struct MgPrepared {
    bool ok = false;
    pgo_mg::Hierarchy H;
    std::vector<double> inv_cnt;                          // several ranks: 1 / members of every level-1 node (uploaded to M.inv_cnt)
    std::vector<int32_t> pi32; std::vector<int64_t> pi64; size_t nf64 = 0;      // the pools (the fp64 one starts zeroed)
    enum Pool { I32, I64, F64 };
    struct Reloc { void* field; Pool pool; size_t off; };
    std::vector<Reloc> reloc;
    // the descriptors
    MgDev M{}; MgLevelDev levels[MG_MAX_LEVELS]{};
    bool fine = false; MgLevelDev fineF{}, fineT{};      // smoothed keyframe transition: the keyframe level's set-up view and transfer view
    std::vector<pgo_mg::ExchangePlan> plans; std::vector<LevelPlanDev> lvl_plan;      // several ranks: the cycle's level plans (plans[l]: level l+1; the last: the dense level's residual)
    pgo_mg::SetupPlans setup; std::vector<SetupPlanDev> su_plan;                      // several ranks, distributed set-up: the block exchanges of every distributed level
    int32_t fw_row0 = 0, fw_row1 = 0; int64_t fw_blk0 = 0, fw_blk1 = 0;
    std::vector<uint8_t> dist; std::vector<OwnRange> own;
    int levels_distributed = 0; int64_t rows_total = 0, rows_own = 0, blocks_total = 0, blocks_own = 0;
    std::vector<double> sw_built;          // [Es] s^2 of every switchable edge this hierarchy was matched with
    double moved = 0.0, of_edges = 0.0, host_ms = 0.0;
};
void MgPreparedFree::operator()(MgPrepared* Q) const { delete Q; }

namespace {

// The aggregation multigrid's hierarchy for the graph of this handle and the given switch values (host array over the caller's switches, or null): host-side structure
// (pgo_mg_host.hpp), pooled device arrays, level descriptors.  Called for a graph build, and again inside a solve when the switch values have moved far from the ones the
// hierarchy was built with (regroup): the levels above level 1 are matched along the couplings that are alive NOW.  p->mg.cache keeps what does not depend on the switches.
// Reads the handle's edge lists, options and mg.cache only (single rank: no HIP, no collective -> may run on a worker thread)
int mg_prepare_impl(pgo_problem* p, const double* sw_now, MgPrepared& Q);
// block -> row of a block-CSR pattern
std::vector<int32_t> row_index(const std::vector<int32_t>& rowptr) {
    std::vector<int32_t> row(rowptr.empty() ? 0 : (size_t)rowptr.back());
    for (size_t i = 0; i + 1 < rowptr.size(); ++i) std::fill(row.begin() + rowptr[i], row.begin() + rowptr[i + 1], (int32_t)i);
    return row;
}
// (runs on worker threads as well: nothing may escape — the C-ABI never throws, and an exception leaving a std::thread is std::terminate)
int mg_prepare(pgo_problem* p, const double* sw_now, MgPrepared& Q) {
    try { return mg_prepare_impl(p, sw_now, Q); }
    catch (const std::bad_alloc&) { Q.ok = false; return PGO_ERR_OUT_OF_MEMORY; }
    catch (...) { Q.ok = false; return PGO_ERR_OUT_OF_MEMORY; }
}
int mg_prepare_impl(pgo_problem* p, const double* sw_now, MgPrepared& Q) {
    const int64_t N = p->N, Ng = p->N_global, S = p->S;
    const int64_t Er = p->rel.size(), Es = p->swe.size();
    int rc;
    const double t0 = now_s();
    pgo_mg::Hierarchy& H = Q.H;
    pgo_mg::timing() = p->opt.verbosity > 1;
    const int dense_max = std::max(1, std::min(p->opt.mg_dense_max_nodes, 512));
    // smoothed prolongators (denser coarse operators, two more row products per cycle on each such level) pay while the coarse levels are latency-bound: measured
    // C4 (200k keyframes) 3.56 -> 2.37 s, C5 (1M keyframes, level 1 = 125k nodes: bandwidth-bound) 8.5 -> 11.1 s.  -1 = by size; with them aggregates of 4 above level 1, else of 8
    const double loop_discount = std::max(0.0, p->opt.mg_loop_discount);
    const int n_smoothed = p->opt.mg_smoothed_levels < 0 ? (Ng <= 500000 ? 1 : 0) : std::min(p->opt.mg_smoothed_levels, MG_MAX_LEVELS);
    const int passes0 = std::max(1, std::min(p->opt.mg_first_passes, 3)), passes = p->opt.mg_passes <= 0 ? (n_smoothed > 0 ? 2 : 3) : std::min(p->opt.mg_passes, 3);
    std::vector<double> sw_w;
    if (sw_now && S > 0) { sw_w.resize((size_t)Es); for (int64_t e = 0; e < Es; ++e) { const double sv = sw_now[p->swe.sw[e]]; sw_w[e] = sv * sv; } }
    Q.sw_built.assign((size_t)Es, 1.0);
    if (!sw_w.empty()) Q.sw_built = sw_w;
    bool ok;
    std::vector<int32_t> agg0_l, mem0_ptr_l, mem0_l;      // several ranks: the keyframe-indexed arrays in the handle's local numbering
    std::vector<double>& inv_cnt = Q.inv_cnt;
    std::vector<int64_t> fine_rowptr, fine_ent; std::vector<int32_t> fine_col;
    // smoothed keyframe transition (one GPU): 1 = on, 0 = off, < 0 = BY THE DENSITY OF THE LEVELS IT MAKES (round 6).  It halves the multigrid iterations everywhere and pays
    // while its denser levels are still latency-sized: over the eight graph types measured in round 5 the sparse levels of the smoothed hierarchy hold 43 000 - 375 000 blocks where
    // it wins (+9 ... +52 %) and 714 000 - 3.9 M where it loses (-19 ... -43 %).  So the hierarchy is built WITH it (graphs beyond 80 000 keyframes are not tried: C3's 100 000 give
    // 734 000 blocks), its blocks are counted, and above SMOOTHED_FINE_MAX_BLOCKS it is built again without (level-0 matching and level-1 structure come from the cache; all of
    // this runs on the worker thread beside build_graph).  Decided once per graph build — a regroup keeps the decision.
    // The limit: round 5's eight graph types are separated by anything between 375 000 and 714 000; round 6's soak of 36 random graphs of 5 000 - 80 000 keyframes
    // (scripts/gpu_mid_soak.py, profiles/r06_mid_soak.txt) found the zone in between mixed — 300 000 blocks -28 % (10 000 keyframes, f = 1..5 + yaw, plain loops), 351 000 +4.5 %,
    // 371 000 -24 %, 375 000 +18 % — and nothing below 280 000 that loses: a missed gain costs less than a regression, so the limit sits under the mixed zone.
    constexpr int64_t SMOOTHED_FINE_MAX_BLOCKS = 280000, SMOOTHED_FINE_TRY_MAX_KEYFRAMES = 80000;
    bool want_fine = !p->local_ids && (p->opt.mg_smoothed_fine > 0 || (p->opt.mg_smoothed_fine < 0 && (p->mg.fine_auto == 1 || (p->mg.fine_auto < 0 && Ng <= SMOOTHED_FINE_TRY_MAX_KEYFRAMES))));
    const bool fine_on_trial = want_fine && p->opt.mg_smoothed_fine < 0 && p->mg.fine_auto < 0;
    auto fine_pattern = [&]() {
        // the keyframe level's block pattern: row i = block (i, i), then one block per incident edge (relative-pose edges first, each class in edge order), and what each block IS for
        // fine_block_value (kind 0: the keyframe's reduced diagonal block; 1 / 2: a relative-pose edge seen from its first / second keyframe; 3 / 4: a switchable edge)
        fine_rowptr.assign((size_t)N + 1, 0);
        for (int64_t e = 0; e < Er; ++e) { fine_rowptr[(size_t)p->rel.c1[e] + 1]++; fine_rowptr[(size_t)p->rel.c2[e] + 1]++; }
        for (int64_t e = 0; e < Es; ++e) { fine_rowptr[(size_t)p->swe.c1[e] + 1]++; fine_rowptr[(size_t)p->swe.c2[e] + 1]++; }
        for (int64_t n = 0; n < N; ++n) fine_rowptr[(size_t)n + 1] += fine_rowptr[n] + 1;
        fine_col.resize((size_t)fine_rowptr[N]); fine_ent.resize((size_t)fine_rowptr[N]);
        std::vector<int64_t> fillb((size_t)N);
        for (int64_t n = 0; n < N; ++n) { fine_col[(size_t)fine_rowptr[n]] = (int32_t)n; fine_ent[(size_t)fine_rowptr[n]] = (n << 3) | 0; fillb[n] = fine_rowptr[n] + 1; }
        auto add = [&](int64_t e, int32_t a, int32_t b, int kind) {
            fine_col[(size_t)fillb[a]] = b; fine_ent[(size_t)fillb[a]++] = (e << 3) | kind;
            fine_col[(size_t)fillb[b]] = a; fine_ent[(size_t)fillb[b]++] = (e << 3) | (kind + 1);
        };
        for (int64_t e = 0; e < Er; ++e) add(e, p->rel.c1[e], p->rel.c2[e], 1);
        for (int64_t e = 0; e < Es; ++e) add(e, p->swe.c1[e], p->swe.c2[e], 3);
    };
    if (want_fine) fine_pattern();
    // filtered smoothed keyframe transition: the blocks that enter the prolongator — the keyframe's own block and its relative-pose (odometry) edges; switchable loop closures do not
    std::vector<uint8_t> fine_keep;
    const bool filtered = want_fine && p->opt.mg_fine_filter != 0 && Es > 0;
    if (filtered) { fine_keep.resize(fine_ent.size()); for (size_t k = 0; k < fine_ent.size(); ++k) fine_keep[k] = (fine_ent[k] & 7) <= 2 ? 1 : 0; }
    if (!p->local_ids) {
        ok = pgo_mg::build_hierarchy(N, p->h_node_free, p->rel.c1, p->rel.c2, p->rel.meas.data() + 7, 8, p->swe.c1, p->swe.c2, sw_w.empty() ? nullptr : sw_w.data(), passes0, passes, dense_max, MG_TILE_ROWS,
                                     MG_MAX_LEVELS, H, false, MG_BLOCK0, nullptr, n_smoothed, loop_discount, &p->mg.cache, want_fine ? &fine_rowptr : nullptr, want_fine ? &fine_col : nullptr,
                                     nullptr, filtered ? &fine_keep : nullptr);
        if (fine_on_trial) {
            int64_t blocks = 0;
            if (ok) for (size_t l = 0; l + 1 < H.L.size(); ++l) blocks += (int64_t)H.L[l].col.size();
            const bool keep = ok && blocks <= SMOOTHED_FINE_MAX_BLOCKS;
            if (p->opt.verbosity > 0) std::fprintf(stderr, "[pgo] multigrid: smoothed keyframe transition on trial: its sparse levels hold %lld blocks (limit %lld) -> %s\n", (long long)blocks, (long long)SMOOTHED_FINE_MAX_BLOCKS, keep ? "kept" : "not used");
            p->mg.fine_auto = keep ? 1 : 0;
            if (!keep) {
                want_fine = false;
                ok = pgo_mg::build_hierarchy(N, p->h_node_free, p->rel.c1, p->rel.c2, p->rel.meas.data() + 7, 8, p->swe.c1, p->swe.c2, sw_w.empty() ? nullptr : sw_w.data(), passes0, passes, dense_max, MG_TILE_ROWS,
                                             MG_MAX_LEVELS, H, false, MG_BLOCK0, nullptr, n_smoothed, loop_discount, &p->mg.cache, nullptr, nullptr);
            }
        }
    } else {
        // Several ranks: every rank gathers the endpoints and weights of ALL edges (one all-reduce of a zero-padded buffer: 24 B per edge, once per graph build)
        // and builds the same hierarchy from the global graph; its own edges and owned keyframes are what it contributes to level 1 (pgo_mg_host.hpp).
        std::vector<double> cnt((size_t)2 * p->world(), 0.0);
        cnt[(size_t)2 * p->rank()] = (double)Er; cnt[(size_t)2 * p->rank() + 1] = (double)Es;
        if ((rc = host_allreduce(p, cnt, 0)) != PGO_OK) return rc;
        int64_t ErT = 0, EsT = 0, my_r = 0, my_s = 0;
        for (int r = 0; r < p->world(); ++r) { if (r == p->rank()) { my_r = ErT; my_s = EsT; } ErT += (int64_t)(cnt[(size_t)2 * r] + 0.5); EsT += (int64_t)(cnt[(size_t)2 * r + 1] + 0.5); }
        std::vector<double> buf((size_t)3 * (ErT + EsT), 0.0);
        double* b_rc1 = buf.data(); double* b_rc2 = b_rc1 + ErT; double* b_rw = b_rc2 + ErT; double* b_sc1 = b_rw + ErT; double* b_sc2 = b_sc1 + EsT; double* b_sw = b_sc2 + EsT;
        for (int64_t e = 0; e < Er; ++e) { b_rc1[my_r + e] = p->rel.c1[e]; b_rc2[my_r + e] = p->rel.c2[e]; b_rw[my_r + e] = p->rel.meas[(size_t)8 * e + 7]; }
        for (int64_t e = 0; e < Es; ++e) { b_sc1[my_s + e] = p->swe.c1[e]; b_sc2[my_s + e] = p->swe.c2[e]; b_sw[my_s + e] = sw_w.empty() ? 1.0 : sw_w[e]; }
        if ((rc = host_allreduce(p, buf, 0)) != PGO_OK) return rc;
        std::vector<int32_t> grc1((size_t)ErT), grc2((size_t)ErT), gsc1((size_t)EsT), gsc2((size_t)EsT);
        std::vector<double> grw(b_rw, b_rw + ErT), gsw(b_sw, b_sw + EsT);
        for (int64_t e = 0; e < ErT; ++e) { grc1[e] = (int32_t)(b_rc1[e] + 0.5); grc2[e] = (int32_t)(b_rc2[e] + 0.5); }
        for (int64_t e = 0; e < EsT; ++e) { gsc1[e] = (int32_t)(b_sc1[e] + 0.5); gsc2[e] = (int32_t)(b_sc2[e] + 0.5); }
        std::vector<uint8_t> gfree((size_t)Ng);
        for (int64_t g = 0; g < Ng; ++g) gfree[g] = p->h_touched_any[g];
        for (int32_t c : p->constant_nodes) if (c >= 0 && c < Ng) gfree[c] = 0;
        const pgo_mg::LocalContrib local{&p->l2g, &p->h_own, &p->rel.c1, &p->rel.c2, &p->swe.c1, &p->swe.c2};
        // distributed cycle: aggregates never mix owners, every level is numbered owner-major (pgo_mg_host.hpp: Owners)
        pgo_mg::Owners OW; OW.touch_mask = &p->h_touch_mask; OW.owner = &p->h_owner; OW.world = p->world(); OW.dist_min_rows = p->opt.mg_dist_min_rows > 0 ? p->opt.mg_dist_min_rows : 8192;
        ok = pgo_mg::build_hierarchy(Ng, gfree, grc1, grc2, grw.data(), 1, gsc1, gsc2, (sw_now && S > 0) ? gsw.data() : nullptr, passes0, passes, dense_max, MG_TILE_ROWS, MG_MAX_LEVELS, H, false, 0, &local, n_smoothed, loop_discount, &p->mg.cache,
                                     nullptr, nullptr, p->world() > 1 ? &OW : nullptr);
        if (ok && p->world() > 1) {
            // the cycle's plans, and beside them on a thread of its own — the two read the finished hierarchy and write their own results — the set-up's (the set-up distributed
            // like the cycle: who contributes to / needs which blocks; the gathered edge lists are rank by rank)
            const bool want_setup = p->opt.mg_dist_setup != 0;
            std::vector<int64_t> rel_off((size_t)p->world() + 1, 0), sw_off((size_t)p->world() + 1, 0);
            for (int r = 0; r < p->world(); ++r) { rel_off[(size_t)r + 1] = rel_off[(size_t)r] + (int64_t)(cnt[(size_t)2 * r] + 0.5); sw_off[(size_t)r + 1] = sw_off[(size_t)r] + (int64_t)(cnt[(size_t)2 * r + 1] + 0.5); }
            const bool tm = pgo_mg::timing();
            std::atomic<bool> worker_failed{false};      // (declared before the thread and its joiner: destroyed after them)
            std::thread worker;
            struct Join { std::thread& t; ~Join() { if (t.joinable()) t.join(); } } join_worker{worker};
            bool started = false;
            if (want_setup && pgo_mg::host_threads() > 1) {
                try {
                    worker = std::thread([&]() { try { pgo_mg::timing() = tm; pgo_mg::build_setup_plans(H, p->rank(), p->world(), grc1, grc2, rel_off, gsc1, gsc2, sw_off, Q.setup); } catch (...) { worker_failed.store(true); } });
                    started = true;
                } catch (...) {}
            }
            pgo_mg::build_level_plans(H, OW, p->rank(), Q.plans);
            if (started) { worker.join(); if (worker_failed.load()) throw std::bad_alloc(); }
            else if (want_setup) pgo_mg::build_setup_plans(H, p->rank(), p->world(), grc1, grc2, rel_off, gsc1, gsc2, sw_off, Q.setup);
        }
        if (ok) {
            const int32_t n1g = (int32_t)H.mem0_ptr.size() - 1;
            inv_cnt.resize((size_t)n1g);
            for (int32_t a = 0; a < n1g; ++a) inv_cnt[a] = 1.0 / (double)std::max(1, H.mem0_ptr[a + 1] - H.mem0_ptr[a]);
            agg0_l.resize((size_t)N); mem0_ptr_l.assign((size_t)n1g + 1, 0);
            for (int64_t l = 0; l < N; ++l) { agg0_l[l] = p->h_node_free[l] ? H.agg0[p->l2g[l]] : -1; if (agg0_l[l] >= 0) mem0_ptr_l[(size_t)agg0_l[l] + 1]++; }
            for (int32_t a = 0; a < n1g; ++a) mem0_ptr_l[(size_t)a + 1] += mem0_ptr_l[a];
            mem0_l.resize((size_t)mem0_ptr_l[n1g]);
            std::vector<int32_t> fillm(mem0_ptr_l.begin(), mem0_ptr_l.end() - 1);
            for (int64_t l = 0; l < N; ++l) if (agg0_l[l] >= 0) mem0_l[(size_t)fillm[agg0_l[l]]++] = (int32_t)l;
        }
    }
    Q.ok = ok;
    if (!ok) return PGO_OK;
    const std::vector<int32_t>& A0 = p->local_ids ? agg0_l : H.agg0;
    const std::vector<int32_t>& M0P = p->local_ids ? mem0_ptr_l : H.mem0_ptr;
    const std::vector<int32_t>& M0 = p->local_ids ? mem0_l : H.mem0;
    const int nl = (int)H.L.size();
    const bool dist = H.world > 1;
    const int rank = p->rank();
    // the explicit transfer operator of smoothed transitions (several ranks: always — the implicit form would need two more exchanges per level)
    const bool expl = p->opt.mg_explicit_transfer != 0 || p->local_ids;
    std::vector<int32_t>& pi32 = Q.pi32; std::vector<int64_t>& pi64 = Q.pi64;
    {   // one allocation per pool (the arrays are appended one by one: without the reservation the 10-MB pools are reallocated and copied a dozen times)
        size_t n32 = A0.size() + M0P.size() + M0.size() + (size_t)((N + MG_BLOCK0 - 1) / MG_BLOCK0) * MG_BLOCK0 * 4 + 64, n64 = 0;
        for (const pgo_mg::HostLevel& A : H.L) {
            const size_t tiles = A.tile_agg0.empty() ? 0 : A.tile_agg0.size() - 1;
            n32 += 3 * A.col.size() + A.parent.size() + A.agg_ptr.size() + tiles * (4 + 2 * (size_t)MG_TILE_ROWS) + A.ps_rowptr.size() + 2 * A.ps_col.size() + A.w_rowptr.size() + 5 * A.w_col.size() + (A.smoothed ? tiles * 2 * (size_t)MG_TILE_ROWS + ((size_t)A.rT_rowptr.size() / 4 + 2) * 2 * (size_t)MG_TILE_ROWS : 0) + 16;
            n64 += A.rowptr.size() + A.g_ptr.size() + A.g_ent.size() + A.psT_ptr.size() + A.psT_ent.size();
        }
        if (H.fine_smoothed) {
            const pgo_mg::HostLevel& F = H.F;
            n32 += F.col.size() + F.ps_rowptr.size() + 4 * F.ps_col.size() + F.w_rowptr.size() + 2 * F.w_col.size() + ((size_t)H.L[0].n / 4 + 2) * 2 * (size_t)MG_TILE_ROWS + 16;
            n64 += F.rowptr.size() + F.col.size() + F.psT_ptr.size() + F.psT_ent.size();
        }
        pi32.reserve(n32); pi64.reserve(n64);
    }
    // pooled arrays, each appended where the descriptor field that points to it is named (`field`: a pointer member of Q's descriptors, null: none); doubles rounded up
    // to even counts (16-B loads)
    auto rel = [&](void* field, MgPrepared::Pool pool, size_t off) { if (field) Q.reloc.push_back({field, pool, off}); };
    auto put32 = [&](const std::vector<int32_t>& v, void* field) { const size_t o = pi32.size(); pi32.insert(pi32.end(), v.begin(), v.end()); rel(field, MgPrepared::I32, o); return o; };
    auto put64 = [&](const std::vector<int64_t>& v, void* field) { rel(field, MgPrepared::I64, pi64.size()); pi64.insert(pi64.end(), v.begin(), v.end()); };
    auto take = [&](size_t cnt, void* field) { const size_t o = Q.nf64; Q.nf64 += (cnt + 1) & ~(size_t)1; rel(field, MgPrepared::F64, o); return o; };
    auto align32 = [&](size_t k) { while (pi32.size() % k) pi32.push_back(0); };
    MgDev& M = Q.M;
    M.n_levels = nl; M.n1 = H.L[0].n;
    M.a0 = dist ? H.L[0].own_ptr[(size_t)rank] : 0; M.a1 = dist ? H.L[0].own_ptr[(size_t)rank + 1] : H.L[0].n;      // the rank's own level-1 aggregates
    const size_t o_agg0 = put32(A0, &M.agg0); put32(M0P, &M.mem0_ptr); put32(M0, &M.mem0);
    // slot table of the restriction inside the vector update: per run of MG_BLOCK0 keyframes its aggregates {id, 8 members as run-local bytes}
    bool have_tab = !p->local_ids && !H.fine_smoothed;      // (smoothed keyframe transition: restriction and prolongation need neighbouring runs — kernels of their own)
    if (have_tab) {
        const int64_t runs = (N + MG_BLOCK0 - 1) / MG_BLOCK0;
        std::vector<int32_t> tab((size_t)runs * MG_BLOCK0 * 4);
        for (size_t k = 0; k < tab.size(); k += 4) { tab[k] = -1; tab[k + 1] = -1; tab[k + 2] = -1; tab[k + 3] = 0; }
        std::vector<int> fill((size_t)runs, 0);
        const int32_t n1h = (int32_t)H.mem0_ptr.size() - 1;
        for (int32_t a = 0; a < n1h && have_tab; ++a) {
            const int32_t m0 = H.mem0_ptr[a], m1 = H.mem0_ptr[a + 1];
            if (m1 <= m0) continue;
            const int64_t run = H.mem0[m0] / MG_BLOCK0;
            if (m1 - m0 > 8 || fill[run] >= MG_BLOCK0) { have_tab = false; break; }
            uint32_t w[2] = {0xffffffffu, 0xffffffffu};
            for (int32_t m = m0; m < m1; ++m) {
                if (H.mem0[m] / MG_BLOCK0 != run) { have_tab = false; break; }
                const int j = m - m0;
                w[j >> 2] = (w[j >> 2] & ~(0xffu << (8 * (j & 3)))) | ((uint32_t)(H.mem0[m] - run * MG_BLOCK0) << (8 * (j & 3)));
            }
            int32_t* e = &tab[((size_t)run * MG_BLOCK0 + fill[run]++) * 4];
            e[0] = a; e[1] = (int32_t)w[0]; e[2] = (int32_t)w[1];
        }
        if (have_tab) { align32(4); put32(tab, &M.blk_tab); }
    }
    const size_t o_d0 = take((size_t)N * 3, &M.d0);
    if (p->local_ids) take((size_t)H.L[0].n, &M.inv_cnt);
    Q.dist.assign((size_t)nl, 0);
    for (int l = 0; l < nl; ++l) {
        const pgo_mg::HostLevel& A = H.L[l];
        MgLevelDev& D = Q.levels[l];
        const bool sparse = l + 1 < nl;
        D.n = A.n; D.n_next = sparse ? H.L[l + 1].n : 0; D.tiles = A.tile_agg0.empty() ? 0 : (int32_t)A.tile_agg0.size() - 1; D.nnzb = (int64_t)A.col.size();
        D.seg_shift = A.seg >= 8 ? 3 : A.seg >= 4 ? 2 : A.seg >= 2 ? 1 : 0;
        D.pad3_ = l;      // (the level's index: read by the timeline variant build only)
        // this rank's rows of the level, once: the cycle's share (several ranks, distributed level: the owner's rows; else all of it) and the set-up's (a distributed level under
        // the distributed set-up forms its own rows, every other one all of them)
        const bool mine = sparse && dist && A.distributed;
        const bool part = l < Q.setup.first_whole;
        const int32_t r0 = mine ? A.own_ptr[(size_t)rank] : 0, r1 = mine ? A.own_ptr[(size_t)rank + 1] : A.n;
        const int32_t s0 = part ? A.own_ptr[(size_t)rank] : 0, s1 = part ? A.own_ptr[(size_t)rank + 1] : A.n;
        Q.dist[(size_t)l] = mine ? 1 : 0;
        if (sparse) {
            D.tile0 = mine ? A.tile_ptr[(size_t)rank] : 0; D.tiles_own = mine ? A.tile_ptr[(size_t)rank + 1] - D.tile0 : D.tiles;
            D.rT_row0 = mine ? H.L[(size_t)l + 1].own_ptr[(size_t)rank] : 0; D.rT_row1 = mine ? H.L[(size_t)l + 1].own_ptr[(size_t)rank + 1] : H.L[(size_t)l + 1].n;
        }
        D.su_row0 = s0; D.su_row1 = s1; D.su_blk0 = A.rowptr[(size_t)s0]; D.su_blk1 = A.rowptr[(size_t)s1];
        OwnRange R;      // (pgo_mg_level_norms: the same ranges whichever way the set-up ran)
        R.row0 = r0; R.row1 = r1; R.blk0 = A.rowptr[(size_t)r0]; R.blk1 = A.rowptr[(size_t)r1];
        if (A.smoothed) {
            D.smoothed = 1; D.n_ps = (int32_t)A.ps_col.size(); D.n_w = (int32_t)A.w_col.size();
            D.su_ps0 = A.ps_rowptr[(size_t)s0]; D.su_ps1 = A.ps_rowptr[(size_t)s1]; D.su_w0 = A.w_rowptr[(size_t)s0]; D.su_w1 = A.w_rowptr[(size_t)s1];
            R.ps0 = A.ps_rowptr[(size_t)r0]; R.ps1 = A.ps_rowptr[(size_t)r1]; R.w0 = A.w_rowptr[(size_t)r0]; R.w1 = A.w_rowptr[(size_t)r1];
            R.rT0 = A.rT_rowptr[(size_t)D.rT_row0]; R.rT1 = A.rT_rowptr[(size_t)D.rT_row1];
        }
        Q.own.push_back(R);
        if (sparse) {      // sharding counters
            if (mine) ++Q.levels_distributed;
            const int64_t blocks = (int64_t)A.col.size() + (A.smoothed ? 2 * (int64_t)A.w_col.size() : 0);
            const int64_t own_blocks = !mine ? blocks : (R.blk1 - R.blk0) + (A.smoothed ? (R.w1 - R.w0) + (R.rT1 - R.rT0) : 0);
            Q.rows_total += A.n; Q.rows_own += r1 - r0; Q.blocks_total += blocks; Q.blocks_own += own_blocks;
        }
        put32(A.col, &D.col); put32(A.parent, &D.parent); put32(A.agg_ptr, &D.agg_ptr);
        {   // block -> row, block -> slot of the transposed block (rows hold the diagonal block first, the others by ascending column)
            std::vector<int32_t> row_of(A.col.size()), tr_of(A.col.size());
            pgo_mg::parallel_ranges(A.n, pgo_mg::host_threads(), [&](int, int32_t lo, int32_t hi) {      // (rows are independent; level 2 of C3 holds 193 000 blocks)
                for (int32_t i = lo; i < hi; ++i)
                    for (int64_t k = A.rowptr[i]; k < A.rowptr[(size_t)i + 1]; ++k) {
                        row_of[(size_t)k] = i;
                        const int32_t j = A.col[(size_t)k];
                        int64_t t = k;
                        if (j != i) {
                            const int32_t* b = A.col.data() + A.rowptr[j] + 1; const int32_t* e = A.col.data() + A.rowptr[(size_t)j + 1];
                            const int32_t* f = std::lower_bound(b, e, i);
                            if (f != e && *f == i) t = f - A.col.data();
                        }
                        tr_of[(size_t)k] = (int32_t)t;
                    }
            });
            put32(row_of, &D.row_of); put32(tr_of, &D.tr_of);
        }
        {   // per tile {a0, a1, i0, i1}, 16-B aligned
            std::vector<int32_t> info;
            for (size_t tt = 0; tt + 1 < A.tile_agg0.size(); ++tt) { const int32_t a0 = A.tile_agg0[tt], a1 = A.tile_agg0[tt + 1]; info.insert(info.end(), {a0, a1, A.agg_ptr[a0], A.agg_ptr[a1]}); }
            align32(4);
            put32(info, &D.tile_info);
            std::vector<int32_t> rows;      // [tile][MG_TILE_ROWS] {first block, end block} of each row of the tile
            for (size_t tt = 0; tt + 1 < A.tile_agg0.size(); ++tt) {
                const int32_t i0 = A.agg_ptr[A.tile_agg0[tt]], i1 = A.agg_ptr[A.tile_agg0[tt + 1]];
                for (int li = 0; li < MG_TILE_ROWS; ++li) { const int32_t r = i0 + li; rows.push_back(r < i1 ? (int32_t)A.rowptr[r] : 0); rows.push_back(r < i1 ? (int32_t)A.rowptr[r + 1] : 0); }
            }
            put32(rows, &D.tile_rows);
        }
        put64(A.rowptr, &D.rowptr); put64(A.g_ptr, &D.g_ptr); put64(A.g_ent, &D.g_ent);
        take(A.col.size() * 36, &D.val); take((size_t)A.n * 36, &D.Dinv); take((size_t)A.n * 3, &D.pos); take((size_t)A.n * 3, &D.d);
        take((size_t)A.n * 6, &D.r); take((size_t)A.n * 6, &D.x); take((size_t)A.n * 6, &D.xt); take((size_t)A.n * 6, &D.xf);
        take((A.col.size() * 36 + 1) / 2, &D.valf);      // fp32 copy of the blocks, carved out of the fp64 pool
        if (A.smoothed) {
            put32(A.ps_rowptr, &D.ps_rowptr); put32(A.ps_col, &D.ps_col); put32(A.w_rowptr, &D.w_rowptr); put32(A.w_col, &D.w_col);
            put64(A.psT_ptr, &D.psT_ptr); put64(A.psT_ent, &D.psT_ent);
            put32(row_index(A.ps_rowptr), &D.ps_row); put32(row_index(A.w_rowptr), &D.w_row);
            take(A.ps_col.size() * 36, &D.ps_val); take(A.w_col.size() * 36, &D.w_val);
            take((size_t)A.n * 6, &D.t); take((size_t)A.n * 6, &D.u); take((size_t)A.n * 6, &D.y); take((size_t)A.n * 6, &D.zero);
            {   // explicit transfer operator: index arrays, per-tile block ranges of R^T (this level's tiles) and of R (tiles of consecutive coarse rows), fp32 block arrays
                put32(A.rT_col, expl ? &D.rT_col : nullptr); put32(A.rT_of_w, expl ? &D.rT_of_w : nullptr); put32(A.ps_of_w, expl ? &D.ps_of_w : nullptr);
                std::vector<int32_t> rows;
                for (size_t tt = 0; tt + 1 < A.tile_agg0.size(); ++tt) {
                    const int32_t i0 = A.agg_ptr[A.tile_agg0[tt]], i1 = A.agg_ptr[A.tile_agg0[tt + 1]];
                    for (int li = 0; li < MG_TILE_ROWS; ++li) { const int32_t r = i0 + li; rows.push_back(r < i1 ? A.w_rowptr[r] : 0); rows.push_back(r < i1 ? A.w_rowptr[(size_t)r + 1] : 0); }
                }
                align32(2);
                put32(rows, expl ? &D.rt_rows : nullptr);
                const int seg_shift = A.rT_seg >= 8 ? 3 : A.rT_seg >= 4 ? 2 : A.rT_seg >= 2 ? 1 : 0;
                const int rpt = MG_TILE_ROWS >> seg_shift;
                const int32_t nb0 = D.rT_row0, nb = D.rT_row1;      // (several ranks: the restriction's tiles cover the rank's own coarse rows)
                const int rT_tiles = (nb - nb0 + rpt - 1) / rpt;
                if (expl) { D.rT_tiles = rT_tiles; D.rT_seg_shift = seg_shift; }
                rows.clear();
                for (int tt = 0; tt < rT_tiles; ++tt)
                    for (int li = 0; li < MG_TILE_ROWS; ++li) { const int32_t r = nb0 + tt * rpt + li; const bool in = li < rpt && r < nb; rows.push_back(in ? A.rT_rowptr[r] : 0); rows.push_back(in ? A.rT_rowptr[(size_t)r + 1] : 0); }
                put32(rows, expl ? &D.rT_rows : nullptr);
                take((A.w_col.size() * 36 + 1) / 2, expl ? &D.rt_valf : nullptr); take((A.w_col.size() * 36 + 1) / 2, expl ? &D.r_valf : nullptr);
            }
        }
    }
    Q.lvl_plan.assign(Q.plans.size(), LevelPlanDev{});
    for (size_t l = 0; l < Q.plans.size(); ++l) { put32(Q.plans[l].send_idx, &Q.lvl_plan[l].send_idx); put32(Q.plans[l].recv_idx, &Q.lvl_plan[l].recv_idx); }
    if (Q.setup.first_whole > 0) {
        const pgo_mg::HostLevel& L1 = H.L[0];
        std::vector<int32_t> g0_slots;
        for (size_t k = 0; k + 1 < L1.g_ptr.size(); ++k) if (L1.g_ptr[k + 1] > L1.g_ptr[k]) g0_slots.push_back((int32_t)k);
        put32(g0_slots, &M.g0_slots); M.n_g0 = (int32_t)g0_slots.size();
        const pgo_mg::HostLevel& W = H.L[(size_t)Q.setup.first_whole];
        Q.fw_row0 = W.own_ptr[(size_t)rank]; Q.fw_row1 = W.own_ptr[(size_t)rank + 1];
        Q.fw_blk0 = W.rowptr[(size_t)Q.fw_row0]; Q.fw_blk1 = W.rowptr[(size_t)Q.fw_row1];
    }
    Q.su_plan.assign(Q.setup.val.size(), SetupPlanDev{});
    for (size_t l = 0; l < Q.setup.val.size(); ++l) {
        SetupPlanDev& so = Q.su_plan[l];
        const pgo_mg::BlockPlan& B = Q.setup.val[l];
        put32(B.x.send_idx, &so.val_send); put32(B.dst, &so.val_dst); put32(B.sum_ptr, &so.val_sum_ptr); put32(B.sum_src, &so.val_sum_src);
        if (l < Q.setup.ps.size()) {
            put32(Q.setup.ps[l].send_idx, &so.ps_send); put32(Q.setup.ps[l].recv_idx, &so.ps_recv); put32(Q.setup.rv[l].send_idx, &so.rv_send); put32(Q.setup.rv[l].recv_idx, &so.rv_recv);
            const bool smoothed = H.L[l].smoothed;      // (the level's set-up is distributed: l < first_whole)
            put32(Q.setup.prod[l], smoothed ? &Q.levels[l].su_prod : nullptr);
            if (smoothed) Q.levels[l].n_su_prod = (int32_t)Q.setup.prod[l].size();
        }
    }
    Q.fine = H.fine_smoothed;
    if (Q.fine) {
        const pgo_mg::HostLevel& Fh = H.F;
        MgLevelDev& F = Q.fineF;
        MgLevelDev& T = Q.fineT;
        const int32_t n1 = H.L[0].n;
        F.n = Fh.n; F.n_next = n1; F.tiles = 0; F.nnzb = (int64_t)Fh.col.size();
        F.tile0 = 0; F.tiles_own = 0; F.rT_row0 = 0; F.rT_row1 = n1;      // (one GPU: the restriction covers every level-1 row)
        F.su_row0 = 0; F.su_row1 = Fh.n; F.su_blk0 = 0; F.su_blk1 = (int64_t)Fh.col.size(); F.su_ps0 = 0; F.su_ps1 = (int32_t)Fh.ps_col.size(); F.su_w0 = 0; F.su_w1 = (int32_t)Fh.w_col.size();
        F.smoothed = 1; F.n_ps = (int32_t)Fh.ps_col.size(); F.n_w = (int32_t)Fh.w_col.size();
        rel(&F.d, MgPrepared::F64, o_d0); rel(&F.parent, MgPrepared::I32, o_agg0);
        // the transfer view: the set-up view, with the explicit operator's fields describing Ps itself (its own pattern by keyframe row; by level-1 row for the restriction)
        T = F;
        put64(Fh.rowptr, &F.rowptr); put64(fine_ent, &F.g_ent); put32(Fh.col, &F.col);
        put32(Fh.ps_rowptr, &F.ps_rowptr); put32(Fh.ps_col, &F.ps_col); put32(Fh.w_rowptr, &F.w_rowptr); put32(Fh.w_col, &F.w_col);
        put64(Fh.psT_ptr, &F.psT_ptr); put64(Fh.psT_ent, &F.psT_ent);
        put32(row_index(Fh.ps_rowptr), &F.ps_row); put32(row_index(Fh.w_rowptr), &F.w_row);
        // Ps by level-1 row (the restriction r_1 = Ps_0^T r runs as the restriction half of mg_sdown_kernel): position e of psT_ent = slot of the transposed block
        std::vector<int32_t> rT_of_ps(Fh.ps_col.size()), rT_col(Fh.ps_col.size());
        for (size_t e = 0; e < Fh.psT_ent.size(); ++e) { rT_of_ps[(size_t)(Fh.psT_ent[e] & 0xffffffffll)] = (int32_t)e; rT_col[e] = (int32_t)(Fh.psT_ent[e] >> 32); }
        put32(rT_of_ps, &T.rT_of_w); put32(rT_col, &T.rT_col);
        const double mean_row = (double)Fh.ps_col.size() / (double)std::max(1, n1);
        int seg = 1;
        while (seg < 8 && mean_row > 5.0 * seg) seg *= 2;
        T.rT_seg_shift = seg >= 8 ? 3 : seg >= 4 ? 2 : seg >= 2 ? 1 : 0;
        const int rpt = MG_TILE_ROWS >> T.rT_seg_shift;
        T.rT_tiles = (n1 + rpt - 1) / rpt;
        std::vector<int32_t> rows;
        rows.reserve((size_t)T.rT_tiles * MG_TILE_ROWS * 2);
        for (int tt = 0; tt < T.rT_tiles; ++tt)
            for (int li = 0; li < MG_TILE_ROWS; ++li) { const int32_t r = tt * rpt + li; const bool in = li < rpt && r < n1; rows.push_back(in ? (int32_t)Fh.psT_ptr[r] : 0); rows.push_back(in ? (int32_t)Fh.psT_ptr[(size_t)r + 1] : 0); }
        align32(2);
        put32(rows, &T.rT_rows);
        take(Fh.col.size() * 36, &F.val); take((size_t)Fh.n * 36, &F.Dinv); take(Fh.ps_col.size() * 36, &F.ps_val); take(Fh.w_col.size() * 36, &F.w_val);
        take((Fh.ps_col.size() * 36 + 1) / 2, &T.rt_valf); take((Fh.ps_col.size() * 36 + 1) / 2, &T.r_valf);
        if (filtered && want_fine) take((size_t)Fh.n * 36, &F.dlump);
        // every pointer of the set-up view is the transfer view's too
        const char* f0 = reinterpret_cast<const char*>(&F);
        for (size_t k = 0, n = Q.reloc.size(); k < n; ++k) {
            const char* at = static_cast<const char*>(Q.reloc[k].field);
            if (at >= f0 && at < f0 + sizeof(MgLevelDev)) Q.reloc.push_back({reinterpret_cast<char*>(&T) + (at - f0), Q.reloc[k].pool, Q.reloc[k].off});
        }
    }
    Q.host_ms = (now_s() - t0) * 1e3;
    if (p->opt.verbosity > 1) std::fprintf(stderr, "[pgo] hierarchy (host): pooled arrays + descriptors      (total %.2f ms, %u hardware threads reported)\n", Q.host_ms, std::thread::hardware_concurrency());
    return PGO_OK;
}

// what a new hierarchy replaces: the installed one, and the two-level method (the multigrid replaces it on the graphs that have one)
void mg_reset(pgo_problem* p) {
    MgState& m = p->mg;
    p->coarse.built = false; p->coarse.active = false; p->coarse.K = CoarseDev{};
    m.built = false; m.active = false; m.M = MgDev{}; m.geometry_epoch = 0; m.lvl_plan.clear(); m.su_plan.clear(); m.first_whole = 0; m.own.clear();
}

// device half: pools (re)allocated and uploaded, the recorded pointers rebased onto them, the descriptors copied into the handle.  The stream must not be running multigrid
// kernels of the previous hierarchy.
int mg_install(pgo_problem* p, MgPrepared& Q) {
    MgState& m = p->mg;
    mg_reset(p);
    if (!Q.ok) { if (p->opt.verbosity > 0) std::fprintf(stderr, "[pgo] multigrid: the graph does not coarsen (isolated keyframes?) -> off\n"); return PGO_OK; }
    const pgo_mg::Hierarchy& H = Q.H;
    const int nl = (int)H.L.size();
    const int n_top = H.L[nl - 1].n;
    const int nc = (6 * n_top + 63) / 64 * 64;
    HIPCHK(p, m.i32.ensure(std::max<size_t>(Q.pi32.size(), 1))); HIPCHK(p, m.i64.ensure(std::max<size_t>(Q.pi64.size(), 1))); HIPCHK(p, m.f64.ensure(std::max<size_t>(Q.nf64, 2)));
    HIPCHK(p, p->coarse.d_cAc.ensure((size_t)nc * nc)); HIPCHK(p, p->coarse.d_cAcf.ensure((size_t)nc * nc)); HIPCHK(p, p->coarse.d_crc.ensure((size_t)nc * 2)); HIPCHK(p, p->coarse.d_cscr.ensure((size_t)nc * 64 + 4096)); HIPCHK(p, p->coarse.d_cinfo.ensure(4));
    HIPCHK(p, hipMemcpyAsync(m.i32.p, Q.pi32.data(), Q.pi32.size() * sizeof(int32_t), hipMemcpyHostToDevice, p->st));
    HIPCHK(p, hipMemcpyAsync(m.i64.p, Q.pi64.data(), Q.pi64.size() * sizeof(int64_t), hipMemcpyHostToDevice, p->st));
    HIPCHK(p, hipMemsetAsync(m.f64.p, 0, Q.nf64 * sizeof(double), p->st));
    HIPCHK(p, hipMemsetAsync(p->coarse.d_crc.p, 0, (size_t)nc * 2 * sizeof(double), p->st));
    char* const base[3] = {reinterpret_cast<char*>(m.i32.p), reinterpret_cast<char*>(m.i64.p), reinterpret_cast<char*>(m.f64.p)};
    const size_t elem[3] = {sizeof(int32_t), sizeof(int64_t), sizeof(double)};
    for (const MgPrepared::Reloc& r : Q.reloc) { void* at = base[r.pool] + r.off * elem[r.pool]; std::memcpy(r.field, &at, sizeof(at)); }
    if (!Q.inv_cnt.empty()) HIPCHK(p, hipMemcpyAsync(const_cast<double*>(Q.M.inv_cnt), Q.inv_cnt.data(), Q.inv_cnt.size() * sizeof(double), hipMemcpyHostToDevice, p->st));
    HIPCHK(p, hipStreamSynchronize(p->st));
    m.M = Q.M;
    for (int l = 0; l < nl; ++l) m.levels[l] = Q.levels[l];
    m.fine = Q.fine; m.fineF = Q.fineF; m.fineT = Q.fineT;
    m.dist.swap(Q.dist); m.own.swap(Q.own);
    m.levels_distributed = Q.levels_distributed; m.rows_total = Q.rows_total; m.rows_own = Q.rows_own; m.blocks_total = Q.blocks_total; m.blocks_own = Q.blocks_own;
    // the dense coarsest level shares the buffers of the two-level preconditioner, which the multigrid replaces on this graph
    p->coarse.K.n_agg = n_top; p->coarse.K.nc = nc; p->coarse.K.Ac = p->coarse.d_cAc.p; p->coarse.K.Acf = p->coarse.d_cAcf.p; p->coarse.K.rc = p->coarse.d_crc.p; p->coarse.K.yc = p->coarse.d_crc.p + nc;
    m.built = true;
    m.sw_built.swap(Q.sw_built);
    if (p->opt.verbosity > 0) {
        std::fprintf(stderr, "[pgo] multigrid: %lld keyframes", (long long)p->N);
        for (int l = 0; l < nl; ++l) {
            int64_t longest = 0;
            for (int32_t i = 0; i < H.L[l].n; ++i) longest = std::max<int64_t>(longest, H.L[l].rowptr[(size_t)i + 1] - H.L[l].rowptr[(size_t)i]);
            std::fprintf(stderr, " -> %d (%lld blocks, longest row %lld%s)", H.L[l].n, (long long)H.L[l].col.size(), (long long)longest, H.L[l].smoothed ? ", smoothed prolongator above" : "");
        }
        std::fprintf(stderr, ", coarsest dense %d (host %.1f ms)\n", nc, Q.host_ms);
    }
    // several ranks: the plans' segment bounds stay on the host (the vectors are swapped: the elements keep their addresses)
    m.plans.swap(Q.plans);
    m.lvl_plan.swap(Q.lvl_plan);
    for (size_t l = 0; l < m.plans.size(); ++l) m.lvl_plan[l].plan = &m.plans[l];
    m.first_whole = Q.setup.first_whole;
    m.fw_row0 = Q.fw_row0; m.fw_row1 = Q.fw_row1; m.fw_blk0 = Q.fw_blk0; m.fw_blk1 = Q.fw_blk1;
    m.setup = std::move(Q.setup);
    m.su_plan.swap(Q.su_plan);
    return ensure_exchange_buffers(p);
}

// The one host build in flight: started by mg_spawn on a worker thread (inline when no thread is to be had), waited for by whoever needs or drops it.  The worker also frees
// the image installed last: returning ~100 MB to the system costs 5 ms of munmap plus a ~10 ms stall of the next kernels (measured: MMU-notifier invalidations reach the
// GPU's address space), so that happens off the solve's critical path.
void mg_spawn(pgo_problem* p, MgJob::Kind kind, std::vector<double> sw, double moved = 0.0, double of_edges = 0.0) {
    MgJob& J = p->mg.job;
    J.out.reset(new MgPrepared());
    J.out->moved = moved; J.out->of_edges = of_edges;
    J.kind = kind; J.rc = PGO_OK;
    MgPrepared* Q = J.out.get();
    MgPrepared* old = J.old.release();
    auto work = [p, Q, old, sw]() { delete old; p->mg.job.rc = mg_prepare(p, sw.empty() ? nullptr : sw.data(), *Q); };
    try { J.thread = std::thread(work); }
    catch (...) { work(); }      // (the C-ABI never throws)
}
// waits for the build in flight and takes its result (null: it failed, J.rc says how)
MgImage mg_join(pgo_problem* p) {
    MgJob& J = p->mg.job;
    if (J.thread.joinable()) J.thread.join();
    J.kind = MgJob::none;
    MgImage Q = std::move(J.out);
    if (J.rc != PGO_OK) Q.reset();
    return Q;
}

}  // namespace

// the build in flight is not wanted any more (the graph is about to change, the handle to go, or a regroup's solve state is gone): waited for, its result dropped.  A fresh
// graph's is marked for a rebuild (mg.built was an announcement, not a fact); a regroup's leaves the hierarchy in place with its own switch record.
void mg_drop_pending(pgo_problem* p) {
    const bool fresh = p->mg.fresh_pending();
    if (p->mg.job.kind != MgJob::none) mg_join(p);
    if (fresh) { p->mg.built = false; p->graph_dirty = true; }
}

// the caller's keyframe and switch counts decide (the same answer on every rank): graphs with switchable loop closures — all of the reference's — take the multigrid from
// mg_min_keyframes_switchable on, graphs without from mg_min_keyframes; mg_min_keyframes = 0 turns it off altogether
bool wants_multigrid(const pgo_problem* p) {
    if (dense_mode(p)) return false;      // the exact dense solver preconditions nothing: no hierarchy, no worker thread
    int64_t mg_from = p->opt.mg_min_keyframes;
    if (mg_from > 0 && p->S > 0 && p->opt.mg_min_keyframes_switchable > 0) mg_from = std::min<int64_t>(mg_from, p->opt.mg_min_keyframes_switchable);
    return mg_from > 0 && p->N_global >= mg_from;
}

// build_graph, one GPU: the HOST half of the hierarchy (pgo_mg_host.hpp: ~0.1 s for C3, single-threaded sorts and matchings) needs the edge lists and the free flags only, so it
// starts on the worker here and runs beside the rest of build_graph; build_multigrid then only announces it.  Several ranks: its host half holds collectives — built in place.
bool mg_start_fresh(pgo_problem* p, const double* sw_now) {
    p->mg.cache.valid = false; p->mg.fine_auto = -1;
    if (p->local_ids || !wants_multigrid(p)) return false;
    std::vector<double> sw;      // the caller's switch array is only guaranteed to live as long as this call
    if (sw_now && p->S > 0) sw.assign(sw_now, sw_now + p->S);
    mg_spawn(p, MgJob::fresh, std::move(sw));
    return true;
}
// The graph's hierarchy, for the given switch values (host array over the caller's switches, or null).  A fresh build on the worker is announced (mg.built) and installed where
// it is first needed — build_mg (the first LM system that wants multigrid operators), the end of the solve, or the next solve_begin (mg_fresh_install).
int build_multigrid(pgo_problem* p, const double* sw_now) {
    int rc;
    mg_reset(p);
    if (p->mg.fresh_pending()) { p->mg.sw_built.clear(); p->mg.built = true; return PGO_OK; }
    if (wants_multigrid(p)) {
        MgPrepared Q;
        if ((rc = mg_prepare(p, sw_now, Q)) != PGO_OK) return rc;
        if ((rc = mg_install(p, Q)) != PGO_OK) return rc;
    }
    if (p->local_ids && !p->mg.built) { p->mg.lvl_plan.clear(); if ((rc = ensure_exchange_buffers(p)) != PGO_OK) return rc; }
    return PGO_OK;
}
// ... the fresh build is needed now: waited for and installed
int mg_fresh_install(pgo_problem* p) {
    if (!p->mg.fresh_pending()) return PGO_OK;
    const double t0 = now_s();
    MgImage Q = mg_join(p);
    if (!Q) {      // the worker failed: the handle keeps working with what a graph without a hierarchy gets (build_graph's synchronous path does the same)
        p->mg.built = false;
        const int rc_worker = p->mg.job.rc != PGO_OK ? p->mg.job.rc : PGO_ERR_STATE;
        HIPCHK(p, hipStreamSynchronize(p->st));
        const int rc2 = build_two_level_aggregates(p);
        ++p->pcg.build_epoch;
        return rc2 != PGO_OK ? rc2 : rc_worker;
    }
    const double waited = (now_s() - t0) * 1e3;
    int rc;
    HIPCHK(p, hipStreamSynchronize(p->st));
    if ((rc = mg_install(p, *Q)) != PGO_OK) return rc;
    // a hierarchy that does not coarsen: the graph falls back to the two-level method — exactly what build_graph's synchronous path (several ranks) gives the same graph
    if (!p->mg.built && (rc = build_two_level_aggregates(p)) != PGO_OK) return rc;
    ++p->pcg.build_epoch;
    if (p->opt.verbosity > 1) std::fprintf(stderr, "[pgo] multigrid: hierarchy of the new graph installed at its first use: host half %.2f ms on a worker thread, waited %.2f ms, installed in %.2f ms%s\n",
                                           Q->host_ms, waited, (now_s() - t0) * 1e3 - waited, p->mg.built ? "" : " — it does not coarsen: the two-level method on this graph");
    p->mg.job.old = std::move(Q);
    return PGO_OK;
}

// the relaxation weight of the smoothers; c = w_p / w of the smoothed prolongators (Dinv holds w D^-1)
static double mg_omega(const pgo_problem* p) { return p->opt.mg_omega > 0.0 && p->opt.mg_omega <= 1.0 ? p->opt.mg_omega : 0.9; }
double mg_cs(const pgo_problem* p) {
    const double wp = p->opt.mg_prolongation_damping > 0.0 && p->opt.mg_prolongation_damping < 0.85 ? p->opt.mg_prolongation_damping : 0.6;
    return wp / mg_omega(p);
}
const MgLevelDev* mg_fine_view(const pgo_problem* p) { return p->mg.fine ? &p->mg.fineT : nullptr; }      // smoothed keyframe transition: what the cycle restricts and prolongs with
double mg_scale(const pgo_problem* p) { return p->opt.mg_correction_scale >= 1.0 && p->opt.mg_correction_scale <= 4.0 ? p->opt.mg_correction_scale : 1.0; }

// Several ranks: which exchange the multigrid cycle needs at one of launch_mg_apply's hook points (pgo_internal.hpp: MgExchangeHook) — the plan (index of the level whose vectors
// travel) and the one or two vectors; false: none.  Level `lv` (1-based) is "distributed" when its kernels run on the owner's rows only; otherwise every rank runs all its rows.
//   point 0, down-sweep of lv (lv = n_levels: the dense solve):  a distributed level reads x (with an explicit transfer operator also r) on the halo of its rows; a level every
//            rank runs completely needs r and x complete — a gather — when what produced them ran on owned rows only (the level below is distributed, or lv = 1: the restriction
//            from the keyframes covers the rank's own aggregates)
//   point 1, up-sweep of a distributed lv:  plain transition: xt of lv on the halo, unless the level above wrote all of it (a level every rank runs completely, or the dense
//            solve, prolongs into every child it holds a valid x for: own rows + halo); explicit operator: xf of lv + 1 on the columns of R^T, when that level is distributed
//   point 2, prolongation to the keyframes:  xf of level 1 at the aggregates of every keyframe the rank touches, when level 1 is distributed
bool mg_exchange_at(pgo_problem* p, int point, int lv, int* plan, double** v1, double** v2, const double** dinv /* non-null result: only r (*v2) travels, x (*v1) = Dinv r is formed on receipt */) {
    const int nl = p->mg.M.n_levels;
    auto dist = [&](int level) { return level >= 1 && level < nl && (size_t)(level - 1) < p->mg.dist.size() && p->mg.dist[(size_t)level - 1] != 0; };
    auto expl = [&](int level) { return level >= 1 && level < nl && mg_explicit(p->mg.levels[level - 1]); };
    *v1 = nullptr; *v2 = nullptr; *plan = -1; *dinv = nullptr;
    if (p->world() <= 1 || p->mg.lvl_plan.empty()) return false;
    if (point == 0) {
        if (lv == nl) { if (nl == 1 || dist(nl - 1)) { *plan = nl - 1; *v1 = p->coarse.K.rc; return true; } return false; }
        MgLevelDev& A = p->mg.levels[lv - 1];
        if (dist(lv)) { *plan = lv - 1; *v1 = A.x; if (expl(lv)) { *v2 = A.r; *dinv = A.Dinv; } return true; }
        if (lv == 1 || dist(lv - 1)) { *plan = lv - 1; *v1 = A.x; *v2 = A.r; *dinv = A.Dinv; return true; }
        return false;
    }
    if (point == 1) {
        if (!dist(lv)) return false;
        if (expl(lv)) { if (dist(lv + 1)) { *plan = lv; *v1 = p->mg.levels[lv].xf; return true; } return false; }
        if (dist(lv + 1)) { *plan = lv - 1; *v1 = p->mg.levels[lv - 1].xt; return true; }
        return false;
    }
    if (point == 2) { if (nl >= 2 && dist(1)) { *plan = nl; *v1 = p->mg.levels[0].xf; return true; } return false; }      // (the prolongation's own plan: a subset of level 1's halo)
    return false;
}
struct MgHookCtx { pgo_problem* p; const int32_t* stop; };
static int mg_exchange_hook(void* ctx, int point, int level) {
    MgHookCtx* c = static_cast<MgHookCtx*>(ctx);
    int plan; double* v1; double* v2; const double* dinv;
    if (!mg_exchange_at(c->p, point, level, &plan, &v1, &v2, &dinv)) return PGO_OK;
    return exchange_level(c->p, plan, v1, v2, c->stop, dinv);
}
// z += s P V(P^T r) on several ranks: the cycle's kernels on this rank's share of every level, the exchanges their reads need in between
int mg_apply_ranks(pgo_problem* p, bool inside_iteration) {
    MgHookCtx hc{p, inside_iteration ? p->C.flags : nullptr};
    MgExchangeHook hook{&hc, mg_exchange_hook};
    MgCycleArgs a;
    a.inside_iteration = inside_iteration; a.hook = &hook;
    return mg_cycle(p, p->C, a);
}
// One cycle on the handle's hierarchy: what every caller would say alike — the correction scale, c of the smoothed transitions, the keyframe level's transfer view, z — is filled
// in here; r and the r.z partials default to C's (the PCG start); `a` states what differs.  Returns the exchange hook's code.
int mg_cycle(pgo_problem* p, const CgDev& C, MgCycleArgs a) {
    if (!a.r) a.r = C.r;
    if (!a.part_rz) a.part_rz = C.part_rz;
    a.z = C.z; a.scale = mg_scale(p); a.prolong_scale = mg_cs(p); a.fine = mg_fine_view(p);
    return launch_mg_apply(p->G, C, p->mg.M, p->mg.levels, p->coarse.K, a, p->st);
}

// Multigrid operators of the system just built: Galerkin products level by level, block-Jacobi inverses, dense inverse of the coarsest level.
// A block that is not numerically positive definite leaves the multigrid off for this LM iteration (plain block-Jacobi).
// Regroup: the hierarchy was built from the switch values of its time (0.99 everywhere at the first solve of a graph).  A few LM steps later the solver has
// switched the outliers off, and aggregates of the levels above level 1 that such a loop closure held together are no rigid pieces any more: measured on C3, the
// late systems need 305 / 367 / 454 multigrid iterations with the hierarchy of the start against 156 / 187 / 249 with one built from the final switch values.  So when
// multigrid operators are about to be built and the switch values have moved far from the hierarchy's (switchable edges that moved by > 0.5 in s^2 make up more than mg_regroup_fraction of ALL
// edges), the levels above level 1 are matched again along the couplings alive NOW (the keyframes' level-1 aggregates, matched along relative-pose edges only, and the
// level-1 structure are cached: pgo_mg::BuildCache) — at most twice per solve.  Several ranks: the count is all-reduced, every rank regroups at the same LM step.
// how many switchable edges have moved by > 0.5 in s^2 since the hierarchy was matched, against ALL residual blocks (what counts is how much of the coupling structure
// changed: C4 has 2 % loop closures — no regroup pays there); summed over the ranks
static int regroup_count(pgo_problem* p, const double* sv, std::vector<double>& cnt, double moved_by = 0.5) {
    const int64_t Es = p->swe.size();
    cnt.assign(2, 0.0);
    for (int64_t e = 0; e < Es; ++e) { const double w = sv[p->swe.sw[e]] * sv[p->swe.sw[e]]; if (std::fabs(w - p->mg.sw_built[e]) > moved_by) cnt[0] += 1.0; }
    cnt[1] = (double)(Es + p->rel.size());
    return p->local_ids ? host_allreduce(p, cnt, 0) : PGO_OK;
}
// A regroup is TRANSACTIONAL: the hierarchy in place is replaced only by one that coarsened; when the matching along the current couplings stalls (build_hierarchy
// gives up above 0.85 nodes per node, or runs out of levels) the installed hierarchy stays — with the new switch record, so that the same failing attempt is not
// repeated at every later check — instead of the handle silently falling back to plain block-Jacobi for the rest of its life.
static int regroup_commit(pgo_problem* p, MgPrepared& Q) {
    if (!Q.ok) {
        if (p->opt.verbosity > 0) std::fprintf(stderr, "[pgo] multigrid: the regrouped hierarchy does not coarsen -> the one in place stays\n");
        p->mg.sw_built.swap(Q.sw_built);
        return PGO_OK;
    }
    int rc;
    HIPCHK(p, hipStreamSynchronize(p->st));
    if ((rc = mg_install(p, Q)) != PGO_OK) return rc;
    ++p->pcg.build_epoch;      // captured PCG chunks hold pointers into the old pools
    return PGO_OK;
}
int regroup_if_moved(pgo_problem* p, const double* sv /* host: the caller's switch array */, bool in_solve) {
    std::vector<double> cnt;
    int rc;
    if ((rc = regroup_count(p, sv, cnt, in_solve ? 0.5 : 0.0)) != PGO_OK) return rc;
    // inside a solve: once the moved edges are a sizeable part of the coupling structure.  At the START of a solve: whenever ANY switch differs from the record — the
    // hierarchy a solve starts with is then a function of the graph and of the solve's own start values alone, whatever earlier solves of the handle left behind
    // (pgo.h: "no per-handle history"; tests/test_gpu_determinism.py solves from state A after a solve that regrouped and compares with a fresh handle, bit for bit).
    if (in_solve ? !(cnt[0] > p->opt.mg_regroup_fraction * cnt[1]) : !(cnt[0] > 0.0)) return PGO_OK;
    const double t0 = now_s();
    MgPrepared Q;
    if ((rc = mg_prepare(p, sv, Q)) != PGO_OK) return rc;
    if ((rc = regroup_commit(p, Q)) != PGO_OK) return rc;
    if (in_solve) ++p->mg.regroups;
    if (p->opt.verbosity > 0) std::fprintf(stderr, "[pgo] multigrid: regrouped %s (%.0f switchable edges of %.0f edges moved), %.1f ms\n", in_solve ? "inside the solve" : "for the new start", cnt[0], cnt[1], (now_s() - t0) * 1e3);
    return PGO_OK;
}
static bool regroup_allowed(const pgo_problem* p) {
    // (not during the first three LM iterations: the switches of outliers — and of inliers far from the odometry guess, which recover — are still falling then: measured on C3,
    // 17 % of the switchable edges have moved after the first step, and a regroup there is paid twice)
    return p->opt.mg_regroup_fraction > 0.0 && p->mg.built && p->S > 0 && p->mg.regroups < 2 && p->lm.iteration >= 3 && (int64_t)p->mg.sw_built.size() == p->swe.size();
}
// several ranks: the regroup happens where multigrid operators are about to be built, synchronously (its host half holds collectives) — every rank at the same LM step
static int maybe_regroup(pgo_problem* p) {
    if (!regroup_allowed(p) || p->lm.iteration <= 3) return PGO_OK;
    std::vector<double> sv((size_t)p->S);
    HIPCHK(p, hipMemcpyAsync(sv.data(), p->d_swv[p->cur].p, sv.size() * sizeof(double), hipMemcpyDeviceToHost, p->st));
    HIPCHK(p, hipStreamSynchronize(p->st));
    return regroup_if_moved(p, sv.data(), true);
}
// One GPU: the HOST half of a regroup (≈25 ms for C3: matching of the upper levels, structures of the smoothed transition, pooled arrays) starts on a worker thread right
// after the accepted step that moved the switches far enough, and is installed where multigrid operators are next built (regroup_install) — on C3 that is a dozen cheap
// block-Jacobi LM steps later, so the solve never waits for it.  Which step starts it and which step installs it depend on the solve's own history only.
int regroup_start(pgo_problem* p) {
    if (p->local_ids || p->mg.job.kind != MgJob::none || !regroup_allowed(p)) return PGO_OK;
    std::vector<double> sv((size_t)p->S);
    HIPCHK(p, hipMemcpyAsync(sv.data(), p->d_swv[p->cur].p, sv.size() * sizeof(double), hipMemcpyDeviceToHost, p->st));
    HIPCHK(p, hipStreamSynchronize(p->st));
    std::vector<double> cnt;
    int rc;
    if ((rc = regroup_count(p, sv.data(), cnt)) != PGO_OK) return rc;
    if (!(cnt[0] > p->opt.mg_regroup_fraction * cnt[1])) return PGO_OK;
    ++p->mg.regroups;
    mg_spawn(p, MgJob::regroup, std::move(sv), cnt[0], cnt[1]);
    return PGO_OK;
}
static int regroup_install(pgo_problem* p) {
    if (p->mg.job.kind != MgJob::regroup) return PGO_OK;
    const double t0 = now_s();
    MgImage Q = mg_join(p);
    if (!Q) return p->mg.job.rc;
    const double waited = (now_s() - t0) * 1e3;
    int rc;
    if ((rc = regroup_commit(p, *Q)) != PGO_OK) return rc;
    if (p->opt.verbosity > 0) std::fprintf(stderr, "[pgo] multigrid: regrouped inside the solve (%.0f switchable edges of %.0f edges moved): host half %.1f ms on a worker thread, waited %.1f ms, installed in %.1f ms\n",
                                           Q->moved, Q->of_edges, Q->host_ms, waited, (now_s() - t0) * 1e3 - waited);
    p->mg.job.old = std::move(Q);      // (not freed here: mg_spawn)
    return PGO_OK;
}

// Several ranks, distributed set-up (round 6): the operators of the current LM system with every DISTRIBUTED level formed by its rows' owners.
//   level 1:  every rank's part of the Galerkin product from its own edges and owned keyframes (mg_operators), then — instead of the all-reduce of ALL of level 1's blocks — the
//             parts of the blocks two ranks share go to the ranks that need them (BlockPlan: summed in ascending rank order)
//   level l distributed:  block-Jacobi inverses, the fp32 copy, the smoother's safety estimate (the whole level's eight power steps on the owners' rows: the iterate's halo before
//             every step, one 3-double all-reduce of the norms and the failure flag — a failed block counts for all ranks); a smoothed transition above it: Dinv of the halo rows (the cycle forms x = Dinv r on receipt), Ps on its own rows, the rows of Ps its rows of W = A Ps
//             multiply from their owners, W and R^T = Ps - Dinv W on its own rows, the blocks of R whose coarse row is another rank's to that rank, its rows' part of Ps^T W to
//             the needers; a plain transition: P^T A P on its own rows (children are the parent's rank's), the blocks above the diagonal also to the column's owner
//   the first level every rank runs completely:  formed like that by its rows' owners, gathered by all; from there on every rank forms the same small levels and the dense inverse
// Nothing here is replicated that grows with the graph: under weak scaling a rank's set-up stays its share + the small top.
static int build_mg_ranks(pgo_problem* p, double omega, int32_t* fail, bool kernels_only) {
    const int fw = p->mg.first_whole;
    int rc;
    if (!kernels_only && (rc = exchange_blocks_sum(p, p->mg.setup.val[0], p->mg.su_plan[0], p->mg.levels[0].val)) != PGO_OK) return rc;
    for (int l = 0; l < fw; ++l) {
        MgLevelDev& A = p->mg.levels[l];
        MgLevelDev& B = p->mg.levels[l + 1];
        launch_mg_level_inverses(A, omega, fail, p->st);
        {   // the smoother's safety estimate: the whole level's power method, the iterate's halo exchanged before every step, the norms (and the failure flag) summed over the ranks
            launch_mg_power_init(A, p->st);
            double* v = A.x; double* w = A.xt;
            for (int it = 0; it < 8; ++it) {
                if (!kernels_only && (rc = exchange_level(p, l, v, nullptr, nullptr, nullptr)) != PGO_OK) return rc;
                launch_mg_power_step(A, v, w, omega, p->st);
                std::swap(v, w);
            }
            launch_mg_power_sums(A, w, v, fail, p->d_xscal.p + 8, p->st);      // (v: 8 steps, w: 7 steps)
            if (!kernels_only && (rc = allreduce(p, p->d_xscal.p + 8, 3, 0)) != PGO_OK) return rc;
            launch_mg_power_finish(p->d_xscal.p + 8, fail, A.xf, p->st);
            launch_mg_level_rescale(A, A.xf, omega, p->st);
        }
        if (A.smoothed) {
            const LevelPlanDev& LP = p->mg.lvl_plan[(size_t)l];
            if (!kernels_only && LP.plan && (rc = exchange_blocks_copy(p, *LP.plan, LP.send_idx, LP.recv_idx, A.Dinv, 36)) != PGO_OK) return rc;
            launch_mg_transition_ps(A, mg_cs(p), p->st);
            if (!kernels_only && (rc = exchange_blocks_copy(p, p->mg.setup.ps[(size_t)l], p->mg.su_plan[(size_t)l].ps_send, p->mg.su_plan[(size_t)l].ps_recv, A.ps_val, 36)) != PGO_OK) return rc;
            launch_mg_transition_w(A, p->st);
            if (!kernels_only && (rc = exchange_blocks_copy(p, p->mg.setup.rv[(size_t)l], p->mg.su_plan[(size_t)l].rv_send, p->mg.su_plan[(size_t)l].rv_recv, reinterpret_cast<double*>(A.r_valf), 18)) != PGO_OK) return rc;
            launch_mg_transition_product(A, B, p->st);
        } else if (l + 1 == fw) {      // the first level every rank runs completely: its own rows here, the rest by the gather below
            MgLevelDev Bo = B;
            Bo.su_row0 = p->mg.fw_row0; Bo.su_row1 = p->mg.fw_row1; Bo.su_blk0 = p->mg.fw_blk0; Bo.su_blk1 = p->mg.fw_blk1;
            launch_mg_level_galerkin(A, Bo, p->st);
        } else launch_mg_level_galerkin(A, B, p->st);
        if (!kernels_only && (rc = exchange_blocks_sum(p, p->mg.setup.val[(size_t)l + 1], p->mg.su_plan[(size_t)l + 1], B.val)) != PGO_OK) return rc;
    }
    return PGO_OK;
}

// The multigrid operators of the current LM system: Galerkin products level by level, block-Jacobi inverses, the dense coarsest level and its inverse (*fail != 0: a block
// that is not numerically positive definite).  kernels_only (pgo_time_kernel(8)): this rank's kernels without the exchanges between them (the numbers are then meaningless).
// t_build0 >= 0 and verbosity > 1: the stream is synchronised after each stage and the time since t_build0 printed.
int mg_operators(pgo_problem* p, int32_t* fail, bool hoff_valid, bool kernels_only, double t_build0) {
    MgState& m = p->mg;
    const double omega = mg_omega(p);
    auto stage = [&](const char* what) -> int {
        if (t_build0 < 0.0 || p->opt.verbosity <= 1) return PGO_OK;
        HIPCHK(p, hipStreamSynchronize(p->st)); std::fprintf(stderr, "[pgo] multigrid: %s done at %.2f ms\n", what, (now_s() - t_build0) * 1e3);
        return PGO_OK;
    };
    int rc;
    if ((rc = stage("geometry")) != PGO_OK) return rc;
    if (m.fine) {      // smoothed keyframe transition: level 1 = Ps_0^T A Ps_0 from the keyframe level's own blocks
        launch_mg_assemble_fine(p->G, p->L, p->Sc, p->C, m.fineF, m.fineT, m.levels[0], omega, fail, p->st, mg_cs(p), hoff_valid, p->d_pose[p->cur].p);
    } else {
        launch_mg_galerkin0(p->G, p->L, p->Sc, p->C, m.M, m.levels, p->st, hoff_valid);
        if ((rc = stage("galerkin0")) != PGO_OK) return rc;
        // several ranks: level 1 = the sum of the ranks' Galerkin products (each edge lives on one rank, each diagonal block is its owner's) — all-reduced, or formed by the
        // owners of its rows under the distributed set-up; the levels above are replicated from the first one every rank runs completely
        if (p->local_ids && m.first_whole > 0) { if ((rc = build_mg_ranks(p, omega, fail, kernels_only)) != PGO_OK) return rc; }
        else if (p->local_ids && !kernels_only && (rc = allreduce(p, m.levels[0].val, (size_t)m.levels[0].nnzb * 36, 0)) != PGO_OK) return rc;
    }
    launch_mg_assemble_rest(m.M, m.levels, p->coarse.K, omega, fail, p->st, mg_cs(p), m.first_whole);
    if ((rc = stage("level operators")) != PGO_OK) return rc;
    launch_coarse_invert(p->coarse.K, p->coarse.d_cscr.p, fail, p->st);
    return PGO_OK;
}

// Multigrid operators of the system just built.  A block that is not numerically positive definite leaves the multigrid off for this LM iteration (plain block-Jacobi).
int build_mg(pgo_problem* p) {
    MgState& m = p->mg;
    m.active = false;
    if (!m.built) return PGO_OK;
    int rc;
    if ((rc = mg_fresh_install(p)) != PGO_OK) return rc;      // the hierarchy of a fresh graph build is installed where it is first needed
    if (!m.built) return PGO_OK;
    const double t_build0 = now_s();
    if ((rc = p->local_ids ? maybe_regroup(p) : regroup_install(p)) != PGO_OK) return rc;
    if (!m.built) return PGO_OK;
    if (p->opt.verbosity > 1) std::fprintf(stderr, "[pgo] multigrid: build_mg past the regroup at %.2f ms\n", (now_s() - t_build0) * 1e3);
    if (m.geometry_epoch != p->lin_epoch) {              // the aggregates' centroids follow the poses of the current linearisation
        if (p->local_ids) {     // a level-1 node's keyframes live on several ranks: owner-weighted position sums, one all-reduce, then as on one GPU
            launch_mg_geometry0_sum(p->G, m.M, m.levels, p->d_pose[p->cur].p, p->st);
            if ((rc = allreduce(p, m.levels[0].pos, (size_t)m.M.n1 * 3, 0)) != PGO_OK) return rc;
            launch_mg_geometry_finish(p->G, m.M, m.levels, p->d_pose[p->cur].p, p->st);
        } else launch_mg_geometry(p->G, m.M, m.levels, p->d_pose[p->cur].p, p->st);
        m.geometry_epoch = p->lin_epoch;
    }
    int32_t* fail = p->coarse.d_cinfo.p;
    HIPCHK(p, hipMemsetAsync(fail, 0, sizeof(int32_t), p->st));
    // level 1's Galerkin product reads J1^T J2 of every edge: the block-CSR solver has them from K2; under the matrix-free solver they are formed here, once per linearisation
    // that builds multigrid operators (an edge-parallel pass whose Jacobian loads coalesce, ~60 us on C3 — the wavefront-per-block product gathering K1's Jacobians itself,
    // twelve strided loads per lane and contribution, took 0.9 ms)
    bool hoff_valid = !p->built_mf;
    if (p->built_mf && p->d_Hoff.cap >= (size_t)(p->G.rel.Epad + p->G.sw.Epad) * 36) {
        if (p->hoff_epoch != p->lin_epoch) { p->L.Hoff = p->d_Hoff.p; launch_k2_offdiag(p->G, p->L, p->st); p->hoff_epoch = p->lin_epoch; }
        hoff_valid = true;
    }
    if ((rc = mg_operators(p, fail, hoff_valid, false, t_build0)) != PGO_OK) return rc;
    if (debug_break_coarse()) launch_coarse_negate(p->coarse.K, p->st);
    int32_t h = 1;
    HIPCHK(p, hipMemcpyAsync(&h, fail, sizeof(h), hipMemcpyDeviceToHost, p->st));
    HIPCHK(p, hipStreamSynchronize(p->st));
    m.active = h == 0;
    // level 1's up-sweep kernel also prolongs to the keyframes; its workgroups (at most MAX_PARTIALS, each taking every gridDim-th tile) put their r.z partials behind the update kernel's
    // (measured: 1 114 tiles on 1 024 workgroups — C4 — lose 3 % to the ragged second trip against the separate prolongation kernel; 3 907 tiles — C5 — gain 3.5 %)
    const int t1 = m.levels[0].tiles;
    p->C.extra_rz = (m.active && !p->local_ids && !m.fine && m.M.n_levels >= 2 && (t1 <= MAX_PARTIALS || t1 >= 2 * MAX_PARTIALS)) ? std::min<int>(t1, MAX_PARTIALS) : 0;
    if (p->opt.verbosity > 0 && h != 0) std::fprintf(stderr, "[pgo] multigrid: a coarse block is not positive definite at radius %.1e -> off for this iteration\n", p->lm.radius);
    if (p->opt.verbosity > 1) std::fprintf(stderr, "[pgo] multigrid: operators of LM iteration %d built in %.2f ms\n", p->lm.iteration, (now_s() - t_build0) * 1e3);
    return PGO_OK;
}

}  // namespace pgo
