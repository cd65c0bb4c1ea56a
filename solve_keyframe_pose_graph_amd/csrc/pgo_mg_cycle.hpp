// pgo_mg_cycle.hpp — the multigrid V-cycle as a list of steps: which kernels one cycle launches on this hierarchy, in which order, with how many workgroups of their own,
// where the exchanges of several ranks fall between them, and which launches can carry the split update's riders (pgo_internal.hpp: UpdRiderDev).  Host description only: no
// HIP runtime call, nothing but pgo_internal.hpp's structs.  launch_mg_apply (pgo_mg_kernels.hpp) walks the plan and launches; choose_split (pgo_pcg.hip) picks the riders' hosts
// from it; tests/test_mg_cycle_plan.py holds the step lists of the hierarchies' shapes written out.
//
// The cycle of levels 1 .. n_levels (the last one dense), level l's record levels[l - 1]:
//   restriction      r_1 = P_0^T r (restrict0), or Ps_0^T r through the keyframe level's transfer view (restrict_fine: mg_sdown_kernel on a level with no tiles of its own);
//                    dropped when the vector update has formed r_1 already (`restricted`), or when this rank restricts to no aggregate
//   l = 1 .. n-1     exchange point (0, l); then an explicit-transfer level smooths and restricts in ONE launch (sdown: its own tiles + the restriction's), any other level
//                    in one (down) — after a row product of its own (pre_smooth) where its smoothed prolongator is applied implicitly
//   dense solve      exchange point (0, n_levels) first; K.n_agg workgroups
//   l = n-1 .. 1     exchange point (1, l); post_smooth for an implicit smoothed level, then up.  With C.extra_rz > 0 level 1's launch also prolongs to the keyframes (up_fused,
//                    at most MAX_PARTIALS workgroups = its r.z partial slots)
//   prolongation     exchange point (2, 1); then prolong0, or prolong_fine through the transfer view; none after up_fused
// Exchange points are collective: they are steps whether or not this rank launches anything at that level (tiles_own == 0).  A launch can carry riders when it is a down / sdown
// launch with workgroups of its own or an up launch other than the fused one — the CG_BLOCK-sized sparse-level launches between the update and the kernel that adds P_0 x_1 to z.
#pragma once
#include "pgo_internal.hpp"

namespace pgo {

// explicit transfer operator on this level: the down-sweep smooths and restricts in one launch, the up-sweep reads the next level's x itself (nothing is prolonged into the level)
inline bool mg_explicit(const MgLevelDev& A) { return A.smoothed && A.rt_valf != nullptr; }

// what a kernel that restricts to the level above `levels[idx]` writes: r, x = Dinv r of that level — the dense level has its residual only (the solve does the rest)
struct MgTarget { double* r; double* x; const double* Dinv; };
inline MgTarget mg_target_above(const MgDev& M, const MgLevelDev* levels, const CoarseDev& K, int idx /* -1: the keyframes */) {
    if (idx + 2 == M.n_levels) return MgTarget{K.rc, nullptr, nullptr};
    return MgTarget{levels[idx + 1].r, levels[idx + 1].x, levels[idx + 1].Dinv};
}

enum class MgStep : int32_t { restrict0, restrict_fine, pre_smooth, down, sdown, dense_solve, post_smooth, up, up_fused, prolong0, prolong_fine, exchange };

struct MgCycleStep {
    MgStep kind;
    int32_t level;       // 1-based; restriction and prolongation: 1 (the level they write / read), the dense solve: n_levels
    int32_t point;       // exchange steps: the hook's point (pgo_internal.hpp: MgExchangeHook); else -1
    uint32_t grid;       // the launch's own workgroups (riders come on top); exchange steps: 0
    bool rider;          // the launch can carry riders of the split update
};

struct MgCyclePlan {
    // per sparse level at most exchange + pre_smooth + down and exchange + post_smooth + up; restriction, exchange, dense solve, exchange, prolongation around them
    static constexpr int CAPACITY = 6 * (MG_MAX_LEVELS - 1) + 5;
    MgCycleStep steps[CAPACITY];
    int n = 0;
    int n_hosts = 0;     // rider-eligible launches: the e-th of them in step order is host ordinal e (UpdSplit)
    void launch(MgStep kind, int level, uint32_t grid, bool rider = false) { steps[n++] = MgCycleStep{kind, level, -1, grid, rider}; n_hosts += rider ? 1 : 0; }
    void exchange(int point, int level) { steps[n++] = MgCycleStep{MgStep::exchange, level, point, 0u, false}; }
};

// cg_grid: workgroups of the PCG's vector kernels (the prolongation's mapping); fine: the keyframe level's transfer view or null (never together with `restricted` or extra_rz)
inline MgCyclePlan mg_cycle_plan(const MgDev& M, const MgLevelDev* levels, const CoarseDev& K, int extra_rz, int cg_grid, bool restricted, const MgLevelDev* fine) {
    MgCyclePlan P;
    const int nl = M.n_levels;
    const bool fused = extra_rz > 0;
    const int own1 = M.a1 > M.a0 ? M.a1 - M.a0 : 0;      // (several ranks: the rank's own aggregates)
    const uint32_t g1 = (uint32_t)((own1 + MG_TILE_ROWS - 1) / MG_TILE_ROWS);
    if (restricted) {}
    else if (fine) P.launch(MgStep::restrict_fine, 1, (uint32_t)fine->rT_tiles);
    else if (g1 > 0) P.launch(MgStep::restrict0, 1, g1);
    for (int l = 1; l < nl; ++l) {
        const MgLevelDev& A = levels[l - 1];
        P.exchange(0, l);
        if (mg_explicit(A)) { if (A.tiles_own + A.rT_tiles > 0) P.launch(MgStep::sdown, l, (uint32_t)(A.tiles_own + A.rT_tiles), true); continue; }
        if (A.tiles_own == 0) continue;
        if (A.smoothed) P.launch(MgStep::pre_smooth, l, (uint32_t)A.tiles_own);
        P.launch(MgStep::down, l, (uint32_t)A.tiles_own, true);
    }
    P.exchange(0, nl);
    P.launch(MgStep::dense_solve, nl, (uint32_t)K.n_agg);
    for (int l = nl - 1; l >= 1; --l) {
        const MgLevelDev& A = levels[l - 1];
        P.exchange(1, l);
        if (A.tiles_own == 0) continue;
        if (A.smoothed && !mg_explicit(A)) P.launch(MgStep::post_smooth, l, (uint32_t)A.tiles_own);
        if (l == 1 && fused) P.launch(MgStep::up_fused, l, (uint32_t)(A.tiles_own < MAX_PARTIALS ? A.tiles_own : MAX_PARTIALS));
        else P.launch(MgStep::up, l, (uint32_t)A.tiles_own, true);
    }
    P.exchange(2, 1);
    if (fine) P.launch(MgStep::prolong_fine, 1, (uint32_t)cg_grid);
    else if (!fused) P.launch(MgStep::prolong0, 1, (uint32_t)cg_grid);
    return P;
}

}  // namespace pgo
