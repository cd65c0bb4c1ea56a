// pgo_handle.hpp — the problem handle (struct pgo_problem) and what the host translation units share: pgo_solver.hip (LM controller, core C-ABI), pgo_graph.hip (host edge
// lists -> device graph), pgo_shard.hip (everything multi-rank above the transport: rank-local numbering, collectives, exchanges, communicator C-ABI, edge sharding),
// pgo_pcg.hip (the two-level method, the preconditioner of each LM system, the PCG driver), pgo_dense.hip (the dense Cholesky solver), pgo_multigrid.hip (the multigrid preconditioner's host lifecycle: hierarchy build,
// install, regroup, operators of each LM system) and pgo_measure.hip (measurement helpers, test diagnostics).  Internal: not installed.
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "pgo.h"
#include "pgo_internal.hpp"
#include "pgo_lm.hpp"
#include "pgo_mg_cycle.hpp"
#include "pgo_comm.hpp"
#include "pgo_mg_host.hpp"

// (what the translation units share stays inside libpgo: only the C-ABI of pgo.h is exported)
#pragma GCC visibility push(hidden)
namespace pgo {

inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// Debug hooks.  None of them is honoured unless the process ALSO sets PGO_ENABLE_DEBUG_HOOKS=1 (read once per process): a PGO_DEBUG_* variable that leaks into a production
// environment on its own does nothing.  The test suite sets the master switch in tests/conftest.py.
inline bool debug_hooks_enabled() { static const bool on = []() { const char* e = std::getenv("PGO_ENABLE_DEBUG_HOOKS"); return e && e[0] == '1' && e[1] == 0; }(); return on; }
// PGO_DEBUG_POISON=1 (read once per process): every new device allocation is filled with 0xFF bytes — a NaN in every double / float, -1 in every index —
// so that a kernel reading memory nobody wrote fails the same way on every box instead of depending on what the allocation held before (tests/test_gpu_determinism.py runs
// its solves under it and compares the results bit for bit with an unpoisoned run).
inline bool debug_poison() { static const bool on = []() { const char* e = std::getenv("PGO_DEBUG_POISON"); return debug_hooks_enabled() && e && e[0] == '1' && e[1] == 0; }(); return on; }
// PGO_DEBUG_BREAK_COARSE=1 (read at every operator build so that a test can switch it inside one process): the dense coarse inverse of the two-level method /
// of the multigrid's coarsest level is applied with the wrong sign — a preconditioner that is not positive definite, i.e. a forced PCG breakdown.
inline bool debug_break_coarse() { if (!debug_hooks_enabled()) return false; const char* e = std::getenv("PGO_DEBUG_BREAK_COARSE"); return e && e[0] == '1' && e[1] == 0; }

// PGO_DEBUG_BREAK_DENSE=1 (read at every factorisation, like PGO_DEBUG_BREAK_COARSE): the dense Cholesky factorisation of that LM system reports a failed pivot — the
// kernel of the first diagonal block raises the failure flag it owns, nothing else changes — so that a test can drive the invalid-step path of a dense step.
inline bool debug_break_dense() { if (!debug_hooks_enabled()) return false; const char* e = std::getenv("PGO_DEBUG_BREAK_DENSE"); return e && e[0] == '1' && e[1] == 0; }

// PGO_DEBUG_NO_SPLIT_UPDATE=1 (read once per process): the multigrid PCG keeps the unsplit vector update (cg_update_mg_kernel<true>) where it would split it
// (tests/test_gpu_split_update.py compares the two bit for bit).
inline bool debug_no_split_update() { static const bool on = []() { const char* e = std::getenv("PGO_DEBUG_NO_SPLIT_UPDATE"); return debug_hooks_enabled() && e && e[0] == '1' && e[1] == 0; }(); return on; }
// PGO_DEBUG_SPLIT_HOSTS=<a>,<b> (read once; for scans): the rider-eligible launches of the cycle plan (pgo_mg_cycle.hpp), by ordinal, that carry the split update's two riders, a <= b
// (a == b: one launch carries both); ignored unless both exist on the hierarchy at hand
inline bool debug_split_hosts(int* a, int* b) {
    static const int v = []() {
        const char* e = std::getenv("PGO_DEBUG_SPLIT_HOSTS");
        if (!debug_hooks_enabled() || !e) return -1;
        char* end = nullptr; const long x = std::strtol(e, &end, 10);
        if (!end || *end != ',' || x < 0 || x > 63) return -1;
        const long y = std::strtol(end + 1, &end, 10);
        return (end && *end == 0 && y >= x && y <= 63) ? (int)(x * 64 + y) : -1;
    }();
    if (v < 0) return false;
    *a = v / 64; *b = v % 64;
    return true;
}

// PGO_DEBUG_GRAPH_AFTER=<n> (read once): the PCG captures its chunk as a hipGraph after n eager iterations instead of 192; values that are not an even number in [2, 10^6] are ignored
inline int debug_graph_after() {
    static const int v = []() {
        const char* e = std::getenv("PGO_DEBUG_GRAPH_AFTER");
        if (!debug_hooks_enabled() || !e) return 192;
        char* end = nullptr; const long n = std::strtol(e, &end, 10);
        return (end && *end == 0 && n >= 2 && n <= 1000000 && (n & 1) == 0) ? (int)n : 192;
    }();
    return v;
}

// a device buffer that owns its memory: grown by ensure(), freed when it goes (the handle's buffers when the handle is deleted, a function's scratch at scope exit)
template <class T>
struct DBuf {
    T* p = nullptr;
    size_t cap = 0;
    DBuf() = default;
    DBuf(const DBuf&) = delete;
    DBuf& operator=(const DBuf&) = delete;
    ~DBuf() { if (p) (void)hipFree(p); }
    hipError_t ensure(size_t n) {
        if (n <= cap) return hipSuccess;
        if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
        const size_t want = n + n / 8 + 64;
        hipError_t e = hipMalloc((void**)&p, want * sizeof(T));
        if (e == hipSuccess) cap = want;
        if (e == hipSuccess && debug_poison()) { e = hipMemset(p, 0xFF, want * sizeof(T)); if (e == hipSuccess) e = hipDeviceSynchronize(); }
        return e;
    }
    // room for max(size, 1) elements, then the host vector's contents on `st`: asynchronous — the vector must outlive the caller's next hipStreamSynchronize(st)
    hipError_t upload(const std::vector<T>& v, hipStream_t st) {
        hipError_t e = ensure(v.empty() ? 1 : v.size());
        if (e == hipSuccess && !v.empty()) e = hipMemcpyAsync(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, st);
        return e;
    }
};

// a pair of timing events destroyed on EVERY exit of the function that holds it (the HIPCHK early returns included)
struct EventPair {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t create() { hipError_t e = hipEventCreate(&e0); if (e == hipSuccess) e = hipEventCreate(&e1); return e; }
    ~EventPair() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
};

struct HostClass {
    std::vector<int32_t> c1, c2, sw;
    std::vector<double> meas;   // 8 per edge: q_obs(4) t_obs(3) w
    std::vector<double> loss;   // the encoded robust loss (+a Huber, -a Cauchy, 0 trivial) of edges [0, loss.size()); the edges beyond it — and all
                                // of them while it is empty (no robust edge was ever added) — are trivial
    int64_t size() const { return (int64_t)c1.size(); }
};

// ---- the multigrid's state on the handle (pgo_multigrid.hip)
struct MgPrepared;                                        // host half of a hierarchy build (pgo_multigrid.hip)
struct MgPreparedFree { void operator()(MgPrepared* Q) const; };
using MgImage = std::unique_ptr<MgPrepared, MgPreparedFree>;

// several ranks: a level's exchange (index lists in the int32 pool, segment bounds on the host), the distributed set-up's block exchanges of a level
struct LevelPlanDev { const int32_t* send_idx = nullptr; const int32_t* recv_idx = nullptr; const pgo_mg::ExchangePlan* plan = nullptr; };
struct SetupPlanDev { const int32_t* val_send = nullptr; const int32_t* val_dst = nullptr; const int32_t* val_sum_ptr = nullptr; const int32_t* val_sum_src = nullptr;
                      const int32_t* ps_send = nullptr; const int32_t* ps_recv = nullptr; const int32_t* rv_send = nullptr; const int32_t* rv_recv = nullptr; };
// this rank's rows of a level and the block ranges they span (one GPU, and levels every rank runs completely: everything)
struct OwnRange { int64_t row0 = 0, row1 = 0, blk0 = 0, blk1 = 0, ps0 = 0, ps1 = 0, w0 = 0, w1 = 0, rT0 = 0, rT1 = 0; };

// The one host build that may be in flight: a fresh graph's hierarchy (started at the top of build_graph, installed where it is first needed — build_mg, the end of the solve,
// or the next solve_begin; until then `built` is true, "this graph has a hierarchy", and the level descriptors are empty) or a regroup (started after the accepted step that
// moved the switches, installed where multigrid operators are next built).  Where either is installed depends on the solve's own history, never on timing.
struct MgJob {
    enum Kind { none, fresh, regroup };
    Kind kind = none;
    std::thread thread;
    MgImage out;                          // what the worker fills
    int rc = 0;                           // ... and its return code
    MgImage old;                          // the image installed last: freed by the next worker or with the handle, off the solve's critical path (regroup_install)
};

struct MgState {
    DBuf<double> f64; DBuf<int32_t> i32; DBuf<int64_t> i64;      // the hierarchy's arrays live in three pooled buffers
    MgDev M{}; MgLevelDev levels[MG_MAX_LEVELS];
    bool fine = false; MgLevelDev fineF{}, fineT{};      // smoothed keyframe transition (opt.mg_smoothed_fine): the keyframe level's set-up view and transfer view
    int fine_auto = -1;                    // mg_smoothed_fine < 0: the decision of this graph build (-1 not taken yet, 0 / 1), written by the hierarchy's worker before it is joined
    bool built = false, active = false;
    pgo_mg::BuildCache cache;              // what the hierarchy builder keeps for a regroup of the same graph
    std::vector<double> sw_built;          // [Es] s^2 of every switchable edge the current hierarchy was built with
    int regroups = 0;                      // regroups of this solve
    uint64_t geometry_epoch = 0;
    MgJob job;
    // several ranks: the level exchanges, per sparse level whether its kernels run on the owner's rows only
    std::vector<LevelPlanDev> lvl_plan;
    std::vector<pgo_mg::ExchangePlan> plans;      // the installed hierarchy's level plans (their segment bounds are read at every exchange)
    std::vector<uint8_t> dist;
    // distributed set-up (round 6): levels [0, first_whole) form the numbers of their own rows only, level first_whole is gathered, the rest is set up by every rank;
    // 0: the set-up is replicated (one GPU; level 1 not distributed; pgo_options.mg_dist_setup = 0)
    pgo_mg::SetupPlans setup; int first_whole = 0;
    int32_t fw_row0 = 0, fw_row1 = 0; int64_t fw_blk0 = 0, fw_blk1 = 0;      // this rank's rows / blocks of level first_whole (it forms them, then all ranks gather the level)
    std::vector<SetupPlanDev> su_plan;
    std::vector<OwnRange> own;             // what the rank's cycle kernels read of every level (pgo_mg_level_norms)
    int levels_distributed = 0; int64_t rows_total = 0, rows_own = 0, blocks_total = 0, blocks_own = 0;      // sharding counters
    bool fresh_pending() const { return job.kind == MgJob::fresh; }
};

// ---- the two-level preconditioner's state on the handle (pgo_pcg.hip).  The multigrid's dense coarsest level borrows K and its buffers (pgo_multigrid.hip).
struct CoarseState {
    DBuf<double> d_ccen, d_cd, d_cAc, d_crc, d_cscr;
    DBuf<float> d_cAcf;              // the dense inverse rounded to fp32
    DBuf<int64_t> d_cblk_ptr, d_ccontrib;
    DBuf<int32_t> d_cblk_ab, d_cagg_free, d_cinfo;
    CoarseDev K{};
    bool built = false, active = false;
    // the method's history on this handle, within a solve and across solves: plain values, saved and put back by copy
    struct History {
        int mode = 0;                    // per solve: 0 not yet compared with plain block-Jacobi, 1 keep, 2 dropped (it did not pay on this graph)
        int retests = 0; bool skip_all = false; double drop_radius = 0.0;   // dropped at a small radius: one more comparison once the radius reaches coarse_min_radius
        int backoff = 0, skip = 0;       // a handle that keeps dropping it (incremental triggers on the same kind of graph) retests ever more rarely
        int keep_streak = 0;             // consecutive solves that kept it: the comparison is then repeated only every 4th solve
    } hist;
    uint64_t geometry_epoch = 0;     // the linearisation (lin_epoch) the aggregates' centroids were computed at
};

// ---- the dense Cholesky solver's state on the handle (pgo_dense.hip; PGO_LINEAR_DENSE_CHOLESKY): sized at graph build, released by a graph build for another solver
struct DenseState {
    DBuf<double> A;            // [n][n] row-major: the system, then its factor L on the lower triangle
    DBuf<double> scratch;      // the current panel, k-major (dense_scratch_doubles)
    DBuf<double> vec;          // w [n] (right-hand side, used up by the forward sweep) and y [n]
    DBuf<double> cov; DBuf<int32_t> cov_idx;      // pgo_pose_covariance, pgo_covariance: right-hand sides, panel copy and blocks (dense_cov_doubles), index lists (dense_param_ints); first call
    int n = 0;                 // 6 keyframes-of-the-handle, padded to a multiple of 64
    bool built = false;
};

// the handle's stream.  It goes with the handle, after the PCG's captured graphs and pinned poll buffer (pgo_problem declares it just before PcgState) and before the
// device buffers: the order in which the handle's resources have always been released
struct OwnedStream {
    hipStream_t s = nullptr;
    OwnedStream() = default;
    OwnedStream(const OwnedStream&) = delete;
    OwnedStream& operator=(const OwnedStream&) = delete;
    ~OwnedStream() { if (s) (void)hipStreamDestroy(s); }
    operator hipStream_t() const { return s; }
};

// ---- the PCG driver's state on the handle (pgo_pcg.hip)
struct PcgState {
    // pipelined convergence polling: pinned host copies of {flags[4], scal[4]} for two chunks in flight
    struct Poll { int32_t flags[4]; double scal[4]; };
    Poll* poll = nullptr; hipEvent_t poll_ev[2] = {nullptr, nullptr};      // poll[2]: snapshot at the start of a PCG phase (base point of the convergence-rate estimate)
    // hipGraph of one PCG chunk (launch-bound inner loop); valid for (graph build epoch, tolerance, chunk length, solver)
    // one captured chunk per preconditioner (0 block-Jacobi, 1 two-level, 2 multigrid): the hybrid policy changes between them inside a solve
    struct CapturedChunk { hipGraphExec_t exec = nullptr; int len = 0; uint64_t epoch = 0; double scale = 0.0; bool sr = false; };   // scale: mg_correction_scale is a by-value kernel argument of the captured cycle
    CapturedChunk cg_chunk[3];
    hipGraphExec_t cg_graph = nullptr;   // the one in use (not owned)
    uint64_t build_epoch = 1; bool cg_graph_failed = false;
    double cg_predicted = 0.0;      // block-Jacobi-equivalent iterations predicted for the current LM system (build_system); 0: none
    double cg_prev_equiv = 0.0, cg_prev_radius = 0.0;   // block-Jacobi-equivalent PCG iterations and radius of the last fully solved LM system of this solve
    int mg_switch_at = 400;              // in-flight switch point of the current LM system (build_system)
    int cg_extra = 0;                    // PCG iterations of the current LM step spent before a change of preconditioner
    bool mg_failed = false;              // the multigrid operators of the current system could not be built
    bool mg_start_deferred = false;      // the current system is predicted hard, but its multigrid operators are built only once the step has survived the first early-rejection pause
    PcgState() = default;
    PcgState(const PcgState&) = delete;
    PcgState& operator=(const PcgState&) = delete;
    hipError_t create() {      // pgo_create: the pinned poll buffer and its events
        hipError_t e = hipHostMalloc((void**)&poll, 3 * sizeof(Poll), hipHostMallocDefault);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&poll_ev[0], hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&poll_ev[1], hipEventDisableTiming);
        if (e == hipSuccess) std::memset(poll, 0, 3 * sizeof(Poll));
        return e;
    }
    ~PcgState() {
        for (CapturedChunk& cc : cg_chunk) if (cc.exec) (void)hipGraphExecDestroy(cc.exec);
        if (poll) (void)hipHostFree(poll);
        for (hipEvent_t e : poll_ev) if (e) (void)hipEventDestroy(e);
    }
};

}  // namespace pgo
#pragma GCC visibility pop

using namespace pgo;

struct pgo_problem {
    pgo_options opt;
    int device = 0;
    std::string err;

    HostClass rel, swe;
    std::vector<PriorDev> priors;
    std::vector<int32_t> constant_nodes;
    bool graph_dirty = true, priors_dirty = true;

    // device graph.  N = keyframes this handle works on: all of the caller's (one GPU), or — multi-GPU — only those touched by the
    // rank's own residual blocks, renumbered densely in ascending global order ("rank-local subgraph"); N_global = the caller's count.
    int64_t N = 0, S = 0, N_global = 0;
    bool local_ids = false;
    std::vector<int32_t> l2g, g2l;            // local -> global, global -> local (-1: not touched by this rank)
    std::vector<uint8_t> h_touched_any;       // [N_global] some rank holds a residual block on the keyframe
    std::vector<double> h_own;                // [N] 1.0 where this rank is the keyframe's owner (lowest rank touching it)
    std::vector<double> h_init_q, h_init_t;   // multi-GPU: the caller's state at solve_begin (keyframes no rank touches are returned as given)
    std::vector<uint64_t> h_touch_mask;       // [N_global] bit r: rank r holds a residual block on the keyframe (one all-reduce at graph build)
    std::vector<int32_t> h_owner;             // [N_global] the rank that owns the keyframe: the one holding most of its residual blocks (a second all-reduce), -1: nobody touches it
    pgo_mg::FinePlan fine_plan;               // the keyframes' neighbour exchange: who shares which keyframes with this rank, and the order their parts are summed in
    DBuf<int32_t> d_l2g, d_fp_send, d_fp_shloc, d_fp_sumptr, d_fp_sumsrc;
    DBuf<double> d_own, d_xsend[2], d_xrecv, d_xscal;   // owner weights; send buffers (by collective parity), receive buffer, the iteration's two scalars
    int64_t n_sh_mine = 0, n_sh_global = 0;
    // exchange accounting (pgo_get_sharding_stats)
    int64_t st_exchanges = 0, st_allreduces = 0, st_pcg_iterations = 0; double st_bytes_neighbour = 0.0, st_bytes_allreduce = 0.0;
    DBuf<int32_t> d_rc1, d_rc2, d_sc1, d_sc2, d_sidx, d_bsr_col;
    DBuf<double> d_rmeas, d_smeas;
    DBuf<double> d_rloss, d_rlossc;   // robust loss plane of the relative-pose class and K1's corrector scales (allocated only for a handle with a robust edge)
    DBuf<double> d_sloss, d_slossc;   // ... of the switchable class (allocated only for a handle with a robust switchable edge)
    DBuf<double> d_a_inv_mf;          // [Es] c^2 a_inv, the matrix-free matvec's Schur scale on such a handle (sw_prepare_loss_kernel); ScMf.a_inv points at it
    DBuf<int4> d_rwin, d_swin;
    DBuf<PriorDev> d_prior;
    DBuf<int64_t> d_inc_rowptr, d_inc, d_bsr_rowptr;
    DBuf<uint8_t> d_node_free;
    DBuf<double> d_Jr, d_Js, d_Jp;
    DBuf<double> d_Hd_g;             // Hd [N][36] followed by g [N][6]  (contiguous: one all-reduce)
    DBuf<double> d_Hoff, d_c, d_hss, d_gs;
    DBuf<double> d_scale_p, d_scale_s, d_diag_p, d_diag_s, d_a_inv;
    DBuf<double> d_val, d_Dtot_b;   // Dtot [N][36] followed by b [N][6]
    DBuf<float> d_Lf;
    DBuf<double> d_cgvec;            // x r r2 z p p2 q  (7 x [N][6])
    DBuf<double> d_part;             // partial-sum scratch: several arrays of n_part
    DBuf<double> d_cgpart;           // part_pq [MAX] + part_rz [2][MAX] + scal[4]
    DBuf<int32_t> d_flags;           // cg flags [4] + invert fail [1]
    DBuf<double> d_scal;             // S_N doubles
    DBuf<double> d_pose[2], d_swv[2], d_delta_s, d_io;   // state ping-pong, staging for quat/t
    DBuf<double> d_tmp;
    DBuf<double> d_vio;              // raw VIO poses [n_vio][16] (graph construction, K0)
    DBuf<int32_t> d_vio_idx; DBuf<double> d_vio_meas;   // K0's edge endpoints and measurements of one call
    CoarseState coarse;                    // the two-level preconditioner (pgo_pcg.hip)
    DenseState dense;                      // the dense Cholesky solver (pgo_dense.hip)
    uint64_t lin_epoch = 0;                // counts linearisations (the two-level method's centroids follow the poses)
    MgState mg;                            // the aggregation multigrid (pgo_multigrid.hip)
    uint64_t hoff_epoch = 0;               // linearisation whose J1^T J2 blocks L.Hoff holds (matrix-free solver: formed on demand for the multigrid's level-1 product)
    int64_t n_vio = 0;
    // matrix-free operator
    DBuf<uint32_t> d_einc;
    DBuf<uint32_t> d_einc_slot;
    DBuf<ushort4> d_node_rng;
    DBuf<int64_t> d_tile_inc0;
    DBuf<int32_t> d_einc_other, d_tile_node0, d_tile_sw0, d_node_prior;
    DBuf<double2> d_rec;
    DBuf<double> d_lam;
    MfDev F{};
    bool built_mf = false;
    int64_t mf_pair_lanes = 0, mf_rel_side_lanes = 0, mf_sw_lanes = 0;   // lanes of the matrix-free operator by kind (pgo_time_kernel's bytes)
    int cur = 0;
    int64_t n_part = MAX_PARTIALS;
    std::vector<uint8_t> h_node_free, h_sw_used;
    int64_t nnzb = 0;

    GraphDev G{};
    LinDev L{};
    ScaleDev Sc{};
    ScaleDev ScMf{};                       // what the matrix-free matvec launches receive: Sc, but on a handle with a robust switchable edge a_inv = d_a_inv_mf
    CgDev C{};

    // the open solve: the LM controller's state (pgo_lm.hpp), the scaling's and the clock's
    bool in_solve = false, scale_ready = false;
    LmState lm;
    double t_begin = 0, t_device0 = 0;
    pgo_summary sum;

    // the multi-rank transport (pgo_comm.hpp); none on one GPU
    std::unique_ptr<pgo_comm::Comm> comm;
    int rank() const { return comm ? comm->rank() : 0; }
    int world() const { return comm ? comm->world() : 1; }

    OwnedStream st;                      // (declared here: released after pcg, before everything above)
    PcgState pcg;                        // the PCG driver (pgo_pcg.hip)
};


#define HIPCHK(p, expr) PGO_HIPCHK((p)->err, expr)

#pragma GCC visibility push(hidden)
namespace pgo {

// scalar slots of d_scal
enum { S_COST = 0, S_PRIOR_COST = 1, S_MODEL = 2, S_SW_STEP2 = 3, S_SW_XNORM2 = 4, S_GMAX = 5, S_STEP2 = 6, S_XNORM2 = 7, S_N = 8 };

inline int set_device(pgo_problem* p) { HIPCHK(p, hipSetDevice(p->device)); return PGO_OK; }
inline double* part(pgo_problem* p, int k) { return p->d_part.p + (size_t)k * p->n_part; }      // partial-sum scratch array k

// ---- pgo_graph.hip: host edge lists -> device graph
int add_edges(pgo_problem* p, HostClass& H, int64_t n, const int32_t* c1, const int32_t* c2, const double* T, const double* w, const int32_t* sw, double loss_enc = 0.0);
int build_graph(pgo_problem* p, int64_t N, int64_t S, const double* sw_now);

// ---- pgo_shard.hip: the rank-local subgraph, the collectives and neighbour exchanges (no-ops without a communicator), keyframe arrays local <-> global
int number_rank_local(pgo_problem* p, int64_t n_global, int64_t* n_local);
int allreduce(pgo_problem* p, double* buf, size_t n, int op /*0 sum, 2 max*/);
int host_allreduce(pgo_problem* p, std::vector<double>& v, int op);
int exchange_rows(pgo_problem* p, double* a1, int k1, double* a2, int k2, const int32_t* stop = nullptr);
int exchange_level(pgo_problem* p, int l, double* v1, double* v2, const int32_t* stop, const double* dinv);
int exchange_blocks_copy(pgo_problem* p, const pgo_mg::ExchangePlan& X, const int32_t* send_idx, const int32_t* recv_idx, double* arr, int K);
int exchange_blocks_sum(pgo_problem* p, const pgo_mg::BlockPlan& B, const SetupPlanDev& D, double* arr);
int ensure_exchange_buffers(pgo_problem* p);
int nodes_to_global(pgo_problem* p, const double* dev, int k, double* host_global);
int nodes_from_global(pgo_problem* p, const double* host_global, int k, double* dev);

// ---- pgo_pcg.hip: the two-level method, the preconditioner of each LM system, the PCG driver
int build_two_level_aggregates(pgo_problem* p);
void two_level_solve_begin(pgo_problem* p);
void two_level_solve_end(pgo_problem* p);
int build_coarse(pgo_problem* p, bool force = false);
int build_lm_system(pgo_problem* p, bool* ok);      // the LM system at the current radius with its preconditioner; *ok false: a diagonal block is not positive definite
bool single_reduction(const pgo_problem* p);
// The form of a PCG iteration: its recurrence, and what follows the vector update.  Chosen once per PCG phase (choose_form), again where the in-flight switch installs the multigrid.
struct PcgForm {
    enum Rec { ranks, sr, sr_coarse, classic_mf, classic_csr, classic_coarse };   // several ranks (Chronopoulos-Gear), single-reduction [+ fused two-level], classic [+ fused two-level]
    enum Post { none, mg_cycle, mg_restricted, two_level };                        // the multigrid cycle (restriction inside the update or not), the unfused two-level correction
    Rec rec; Post post;
    int fused_parts;                     // the fused two-level method: the update kernel's r.z partial slots (the dense solve's C.extra_rz follow them)
    UpdSplit split;                      // sr + mg_restricted: the launches of the cycle that carry the half of the update nothing waits for (off: the unsplit kernel)
    bool single_red() const { return rec == sr || rec == sr_coarse; }
    bool fused_coarse() const { return rec == sr_coarse || rec == classic_coarse; }
    bool mg() const { return post == mg_cycle || post == mg_restricted; }
    int precond() const { return mg() ? 2 : (fused_coarse() || post == two_level) ? 1 : 0; }      // 0 block-Jacobi, 1 two-level, 2 multigrid
};
PcgForm choose_form(const pgo_problem* p, bool this_rank_only = false);      // this_rank_only: the rank's own iteration, without exchanges (pgo_time_kernel)
void pcg_matvec(pgo_problem* p, const PcgForm& f, int k, double tol2);
int pcg_update(pgo_problem* p, const PcgForm& f, int k);
int pcg_precond(pgo_problem* p, const PcgForm& f, int k);
int pcg_iteration(pgo_problem* p, const PcgForm& f, int k, double tol2);
int pcg_start(pgo_problem* p, const PcgForm& f, bool warm, double tol2);
struct CgResult { int iterations; bool breakdown; double rel_residual; bool converged; };
// one PCG phase: up to tol (relative); resume >= 0 continues the stopped PCG at that iteration index (device state x, r, z, p and the partial sums are those of `resume`
// completed iterations); warm: start from the previous solution; switch_now: the multigrid takes over from the iterate a pause left; max_iterations 0: opt.cg_max_iterations
struct PcgPhase { double tol; int resume = -1; bool warm = false; bool switch_now = false; int max_iterations = 0; };
int run_pcg(pgo_problem* p, CgResult* res, const PcgPhase& ph);
int finish_system(pgo_problem* p, CgResult* cg, bool evaluated, int* precond_used);

// ---- pgo_dense.hip: the exact dense solver (PGO_LINEAR_DENSE_CHOLESKY)
bool dense_mode(const pgo_problem* p);
int dense_allocate(pgo_problem* p);      // build_graph: the buffers of this graph
void dense_release(pgo_problem* p);      // build_graph for another solver
int dense_step(pgo_problem* p, bool* ok, double* t_factored);      // lm_step: scatter, factor, failure flag, sweeps into C.x
size_t dense_scratch_doubles(int n);
// pgo_pose_covariance, pgo_covariance: the pairs' blocks of the inverse of the undamped system at solve_begin's linearisation, pose and switch blocks, on a block-CSR or a
// matrix-free graph (block ids: a free keyframe, or N + the internal index of a switchable edge; sw_node: per switchable edge its two keyframes, -1 for a constant one) ...
int dense_param_covariance(pgo_problem* p, const std::vector<int32_t>& sw_node, int64_t n_pairs, const int32_t* ia, const int32_t* ib, double* out, bool* ok);
// ... and its launches (the two pgo_dense_spd_*covariance hooks run exactly these): index upload, the right-hand sides (before the factor: they share its failure flag),
// the substitutions and Gram products on the factor.  Buffers: dense_cov_doubles / dense_param_ints; the blocks land at dense_cov_blocks.
struct DcParamPlan;
size_t dense_cov_doubles(int n, int m, int64_t n_pairs);
double* dense_cov_blocks(double* work, int n, int m);
size_t dense_param_ints(int m, int64_t n_pairs, int64_t n_sw);
int dense_param_upload(pgo_problem* p, const DcParamPlan& Q, int64_t n_sw, const int32_t* sw_node, std::vector<int32_t>& staging, int32_t* idx);
int launch_dense_param_rhs(pgo_problem* p, int n, const DcParamPlan& Q, double* work, const int32_t* idx, const double* sw_c, const double* sw_h, int32_t* fail);
void launch_dense_param_covariance(pgo_problem* p, const double* A, int n, const DcParamPlan& Q, double* work, const int32_t* idx, const double* sw_h);
// the launches themselves (n a multiple of 64; pgo_dense_spd_solve runs exactly these)
void launch_dense_scatter(const GraphDev& G, const CgDev& C, double* A, int n, double* w, hipStream_t st);
void launch_dense_factor(double* A, int n, double* scratch, int32_t* fail, bool force_fail, hipStream_t st);
void launch_dense_solve(const double* A, int n, double* w, double* yv, double* x, int n_out, hipStream_t st);

// ---- pgo_multigrid.hip
bool wants_multigrid(const pgo_problem* p);
void mg_drop_pending(pgo_problem* p);
bool mg_start_fresh(pgo_problem* p, const double* sw_now);
int build_multigrid(pgo_problem* p, const double* sw_now);
int mg_fresh_install(pgo_problem* p);
int regroup_if_moved(pgo_problem* p, const double* sv, bool in_solve);
int regroup_start(pgo_problem* p);
int build_mg(pgo_problem* p);
int mg_operators(pgo_problem* p, int32_t* fail, bool hoff_valid, bool kernels_only, double t_build0);
bool mg_exchange_at(pgo_problem* p, int point, int lv, int* plan, double** v1, double** v2, const double** dinv);
int mg_apply_ranks(pgo_problem* p, bool inside_iteration);
int mg_cycle(pgo_problem* p, const CgDev& C, MgCycleArgs a);      // one cycle on the handle's hierarchy; `a`: what differs from the PCG start's cycle on C's vectors
double mg_cs(const pgo_problem* p);
double mg_scale(const pgo_problem* p);
const MgLevelDev* mg_fine_view(const pgo_problem* p);

}  // namespace pgo
#pragma GCC visibility pop
