// Host instantiation of the multigrid cycle's plan (csrc/pgo_mg_cycle.hpp): a hierarchy's device records are filled from a few integers per level — all the plan reads —
// and the steps come back as rows.  Built as a shared object for tests/test_mg_cycle_plan.py, or — with -DMGC_MAIN — as a stand-alone program that reads the same cases from
// standard input, one per line, and prints their rows: the form to run under -fsanitize=address,undefined.
#include "pgo_mg_cycle.hpp"

static const char* kind_name(pgo::MgStep k) {
    switch (k) {
        case pgo::MgStep::restrict0: return "restrict0";
        case pgo::MgStep::restrict_fine: return "restrict_fine";
        case pgo::MgStep::pre_smooth: return "pre_smooth";
        case pgo::MgStep::down: return "down";
        case pgo::MgStep::sdown: return "sdown";
        case pgo::MgStep::dense_solve: return "dense_solve";
        case pgo::MgStep::post_smooth: return "post_smooth";
        case pgo::MgStep::up: return "up";
        case pgo::MgStep::up_fused: return "up_fused";
        case pgo::MgStep::prolong0: return "prolong0";
        case pgo::MgStep::prolong_fine: return "prolong_fine";
        case pgo::MgStep::exchange: return "exchange";
    }
    return "?";
}

extern "C" {
int mgc_capacity() { return pgo::MgCyclePlan::CAPACITY; }
int mgc_max_levels() { return pgo::MG_MAX_LEVELS; }
// lv [n_levels - 1][4]: tiles_own, rT_tiles, smoothed, explicit transfer (rt_valf set) of every sparse level; n1: the level-1 aggregates this rank restricts to;
// fine_rT_tiles < 0: no transfer view of the keyframe level.  rows [capacity][4]: level, point, grid, rider; names [capacity]: the kind.  Returns the number of steps.
int mgc_plan(int n_levels, const int* lv, int n1, int n_agg, int extra_rz, int cg_grid, int restricted, int fine_rT_tiles, int* rows, const char** names, int* n_hosts) {
    static float some_blocks[1];
    pgo::MgDev M{};
    M.n_levels = n_levels; M.a0 = 0; M.a1 = n1;
    pgo::MgLevelDev levels[pgo::MG_MAX_LEVELS] = {};
    for (int l = 0; l + 1 < n_levels; ++l) {
        levels[l].tiles_own = lv[4 * l]; levels[l].tiles = lv[4 * l]; levels[l].rT_tiles = lv[4 * l + 1]; levels[l].smoothed = lv[4 * l + 2];
        levels[l].rt_valf = lv[4 * l + 3] ? some_blocks : nullptr;
    }
    pgo::CoarseDev K{};
    K.n_agg = n_agg;
    pgo::MgLevelDev fine{};
    fine.smoothed = 1; fine.rt_valf = some_blocks; fine.rT_tiles = fine_rT_tiles;
    const pgo::MgCyclePlan P = pgo::mg_cycle_plan(M, levels, K, extra_rz, cg_grid, restricted != 0, fine_rT_tiles >= 0 ? &fine : nullptr);
    for (int i = 0; i < P.n; ++i) {
        const pgo::MgCycleStep& s = P.steps[i];
        rows[4 * i] = s.level; rows[4 * i + 1] = s.point; rows[4 * i + 2] = (int)s.grid; rows[4 * i + 3] = s.rider ? 1 : 0;
        names[i] = kind_name(s.kind);
    }
    *n_hosts = P.n_hosts;
    return P.n;
}
}

#ifdef MGC_MAIN
#include <cstdio>
#include <vector>

// a case per line: n_levels n1 n_agg extra_rz cg_grid restricted fine_rT_tiles, then four integers per sparse level
int main() {
    int n_levels, n1, n_agg, extra_rz, cg_grid, restricted, fine_rT, cases = 0;
    while (std::scanf("%d %d %d %d %d %d %d", &n_levels, &n1, &n_agg, &extra_rz, &cg_grid, &restricted, &fine_rT) == 7) {
        if (n_levels < 1 || n_levels > mgc_max_levels()) { std::printf("bad case\n"); return 2; }
        std::vector<int> lv((size_t)4 * (n_levels - 1));
        for (int& v : lv) if (std::scanf("%d", &v) != 1) { std::printf("bad case\n"); return 2; }
        std::vector<int> rows((size_t)4 * mgc_capacity());
        std::vector<const char*> names((size_t)mgc_capacity());
        int hosts = 0;
        const int n = mgc_plan(n_levels, lv.data(), n1, n_agg, extra_rz, cg_grid, restricted, fine_rT, rows.data(), names.data(), &hosts);
        std::printf("case %d hosts %d:", cases++, hosts);
        for (int i = 0; i < n; ++i) std::printf(" %s,%d,%d,%d,%d", names[i], rows[4 * i], rows[4 * i + 1], rows[4 * i + 2], rows[4 * i + 3]);
        std::printf("\n");
    }
    return cases > 0 ? 0 : 2;
}
#endif
