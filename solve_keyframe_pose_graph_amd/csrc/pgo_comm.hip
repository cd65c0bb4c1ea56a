// pgo_comm.hip — the three transports behind pgo_comm.hpp's Comm, and the C-ABI calls that need no problem handle (pgo_comm_get_unique_id, pgo_local_group_*).
//
// RcclComm: librccl through dlopen (only touched when pgo_comm_init / pgo_comm_get_unique_id is used).  CustomComm: the caller's callbacks.  LocalComm: the in-process group —
// the ranks are handles of ONE process, each driven by its own host thread.  A collective there is a KERNEL that reads the peers' device buffers directly (one GPU: the same
// address space; several GPUs of one process: peer access over xGMI), ordered by HIP events between the handles' streams.  The host threads only meet at a barrier so that every
// rank's event has been recorded before a peer waits on it.  No host staging, no copies through pinned memory.
//
// Protocol of in-process collective number k (every rank issues the same collectives in the same order; parity = k & 1):
//   1. wait (stream) on the peers' done[parity] events: their reads of THIS rank's parity buffer in collective k - 2 are finished — the buffer may be overwritten
//   2. fill the parity buffer (all-reduce: a copy of the operand; exchange: the solver's pack kernel), record ready[parity], publish the pointer
//   3. host barrier
//   4. wait (stream) on the peers' ready[parity], launch the reading kernel (sum / max in rank order, or the peers' segments copied into the receive buffer), record done[parity]
// One barrier per collective: double buffering by parity makes the done events of collective k - 2 visible (they were recorded before their owner entered barrier k - 1).
#include <dlfcn.h>

#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "pgo_comm.hpp"
#include "pgo_internal.hpp"

#define HIPCHK(expr) PGO_HIPCHK(err, expr)

namespace pgo_comm {

// a device buffer of at least n doubles (what it held is not kept)
static int grow(double*& buf, size_t& cap, size_t n, hipStream_t st, std::string& err) {
    if (cap >= n) return PGO_OK;
    HIPCHK(hipStreamSynchronize(st));
    if (buf) (void)hipFree(buf);
    buf = nullptr; cap = 0;
    HIPCHK(hipMalloc((void**)&buf, (n + n / 4 + 64) * sizeof(double)));
    cap = n + n / 4 + 64;
    return PGO_OK;
}

// [src][dst] segments in one buffer: this rank fills row `rank`, the all-reduce fills the rest, column `rank` is what it receives
int Comm::exchange_via_allreduce(const ExchangeView& X, int K, const double* send, double* recv, std::string& err, size_t& reduced) {
    const int W = world_, r = rank_;
    std::vector<int64_t> off((size_t)W * W + 1, 0);
    for (int i = 0; i < W * W; ++i) off[(size_t)i + 1] = off[(size_t)i] + X.pair_cnt[i] * K;
    const size_t total = (size_t)off[(size_t)W * W];
    if (total == 0) return PGO_OK;
    int rc;
    if ((rc = grow(scratch_, scratch_cap_, total, st_, err)) != PGO_OK) return rc;
    HIPCHK(hipMemsetAsync(scratch_, 0, total * sizeof(double), st_));
    for (int q = 0; q < W; ++q) { const int64_t cnt = (X.send_off[q + 1] - X.send_off[q]) * K; if (cnt > 0) HIPCHK(hipMemcpyAsync(scratch_ + off[(size_t)r * W + q], send + X.send_off[q] * K, (size_t)cnt * sizeof(double), hipMemcpyDeviceToDevice, st_)); }
    reduced = total;
    if ((rc = allreduce(scratch_, total, 0, err)) != PGO_OK) return rc;
    for (int q = 0; q < W; ++q) { const int64_t cnt = (X.recv_off[q + 1] - X.recv_off[q]) * K; if (cnt > 0) HIPCHK(hipMemcpyAsync(recv + X.recv_off[q] * K, scratch_ + off[(size_t)q * W + r], (size_t)cnt * sizeof(double), hipMemcpyDeviceToDevice, st_)); }
    return PGO_OK;
}

namespace {

// ---- RCCL ----
struct Rccl {
    struct Uid { char b[128]; };   // ncclUniqueId (NCCL_UNIQUE_ID_BYTES = 128), passed BY VALUE to ncclCommInitRank
    void* h = nullptr;
    int (*GetUniqueId)(void*) = nullptr;
    int (*CommInitRank)(void**, int, Uid, int) = nullptr;
    int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*Send)(const void*, size_t, int, int, void*, hipStream_t) = nullptr;      // ncclSend(buf, count, type, peer, comm, stream)
    int (*Recv)(void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    std::string error(const char* what, int rc) const { return std::string(what) + ": " + (GetErrorString ? GetErrorString(rc) : "error"); }
};

int load_rccl(Rccl& r, std::string& err) {
    if (r.h) return PGO_OK;
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char* n : names) { r.h = dlopen(n, RTLD_NOW | RTLD_GLOBAL); if (r.h) break; }
    if (!r.h) { err = std::string("dlopen(librccl): ") + dlerror(); return PGO_ERR_COMM; }
    r.GetUniqueId = (int (*)(void*))dlsym(r.h, "ncclGetUniqueId");
    r.CommInitRank = (int (*)(void**, int, Rccl::Uid, int))dlsym(r.h, "ncclCommInitRank");
    r.AllReduce = (int (*)(const void*, void*, size_t, int, int, void*, hipStream_t))dlsym(r.h, "ncclAllReduce");
    r.CommDestroy = (int (*)(void*))dlsym(r.h, "ncclCommDestroy");
    r.Send = (int (*)(const void*, size_t, int, int, void*, hipStream_t))dlsym(r.h, "ncclSend");
    r.Recv = (int (*)(void*, size_t, int, int, void*, hipStream_t))dlsym(r.h, "ncclRecv");
    r.GroupStart = (int (*)())dlsym(r.h, "ncclGroupStart");
    r.GroupEnd = (int (*)())dlsym(r.h, "ncclGroupEnd");
    r.GetErrorString = (const char* (*)(int))dlsym(r.h, "ncclGetErrorString");
    if (!r.GetUniqueId || !r.CommInitRank || !r.AllReduce || !r.CommDestroy) { err = "librccl: missing symbols"; return PGO_ERR_COMM; }
    return PGO_OK;
}
Rccl g_rccl_for_id;

struct RcclComm final : Comm {
    RcclComm(int rank, int world, hipStream_t st) : Comm(rank, world, st) {}
    ~RcclComm() override { if (comm) { (void)hipStreamSynchronize(st_); R.CommDestroy(comm); } }
    int allreduce(double* buf, size_t n, int op, std::string& err) override {
        const int rc = R.AllReduce(buf, buf, n, /*ncclDouble*/ 8, op, comm, st_);
        if (rc != 0) { err = R.error("ncclAllReduce", rc); return PGO_ERR_COMM; }
        return PGO_OK;
    }
    // one group of ncclSend / ncclRecv pairs (point-to-point over the xGMI link of each pair)
    int exchange(const ExchangeView& X, int K, const double* send, double* recv, std::string& err, size_t& reduced) override {
        // PGO_EXCHANGE_VIA_ALLREDUCE=1 (read once; a production switch, not a debug hook): RCCL's point-to-point path is bypassed — the safety net for a node where
        // ncclSend / ncclRecv misbehave (this repo's send / receive path has never run between two physical GPUs)
        static const bool via_allreduce = []() { const char* e = std::getenv("PGO_EXCHANGE_VIA_ALLREDUCE"); return e && e[0] == '1' && e[1] == 0; }();
        if (via_allreduce) return exchange_via_allreduce(X, K, send, recv, err, reduced);
        if (!R.Send || !R.Recv || !R.GroupStart || !R.GroupEnd) { err = "librccl lacks ncclSend / ncclRecv / ncclGroupStart / ncclGroupEnd"; return PGO_ERR_COMM; }
        int rc = R.GroupStart();
        for (int q = 0; q < world_ && rc == 0; ++q) {
            if (q == rank_) continue;
            const int64_t ns = (X.send_off[q + 1] - X.send_off[q]) * K, nr = (X.recv_off[q + 1] - X.recv_off[q]) * K;
            if (ns > 0) rc = R.Send(send + X.send_off[q] * K, (size_t)ns, /*ncclDouble*/ 8, q, comm, st_);
            if (rc == 0 && nr > 0) rc = R.Recv(recv + X.recv_off[q] * K, (size_t)nr, 8, q, comm, st_);
        }
        const int rc_end = R.GroupEnd();
        if (rc == 0) rc = rc_end;
        if (rc != 0) { err = R.error("ncclSend / ncclRecv", rc); return PGO_ERR_COMM; }
        return PGO_OK;
    }
    // RCCL supports stream capture.  Opt-in (PGO_RCCL_GRAPH=1): it could only be tried with a 1-rank communicator on the 1-GPU development boxes.
    bool graph_capturable() const override { static const bool on = []() { const char* e = std::getenv("PGO_RCCL_GRAPH"); return e && e[0] == '1'; }(); return on; }
    Rccl R;
    void* comm = nullptr;
};

// ---- caller-supplied collective ----
struct CustomComm final : Comm {
    CustomComm(pgo_allreduce_fn fn, void* ctx, int rank, int world, hipStream_t st) : Comm(rank, world, st), fn(fn), ctx(ctx) {}
    int allreduce(double* buf, size_t n, int op, std::string& err) override {
        if (fn(ctx, buf, (int64_t)n, op, (void*)st_) != 0) { err = "custom all-reduce callback failed"; return PGO_ERR_COMM; }
        return PGO_OK;
    }
    // its exchange callback, or — without one — the exchange emulated through its all-reduce
    int exchange(const ExchangeView& X, int K, const double* send, double* recv, std::string& err, size_t& reduced) override {
        if (!xfn) return exchange_via_allreduce(X, K, send, recv, err, reduced);
        off_send.resize((size_t)world_ + 1); off_recv.resize((size_t)world_ + 1);
        for (int q = 0; q <= world_; ++q) { off_send[(size_t)q] = X.send_off[q] * K; off_recv[(size_t)q] = X.recv_off[q] * K; }
        if (xfn(ctx, send, off_send.data(), recv, off_recv.data(), (void*)st_) != 0) { err = "custom exchange callback failed"; return PGO_ERR_COMM; }
        return PGO_OK;
    }
    bool set_exchange(pgo_exchange_fn f) override { xfn = f; return true; }
    pgo_allreduce_fn fn;
    void* ctx;
    pgo_exchange_fn xfn = nullptr;
    std::vector<int64_t> off_send, off_recv;      // the segment bounds in doubles of the exchange in flight
};

// ---- in-process group ----
constexpr int MAX_RANKS = 16;
static_assert(MAX_RANKS <= (int)(sizeof(pgo::LocalPeers::src) / sizeof(pgo::LocalPeers::src[0])), "a kernel reads at most LocalPeers' peers");

struct Group {
    int world = 0;
    std::mutex m;
    std::condition_variable cv;
    int arrived = 0;
    uint64_t generation = 0;
    bool broken = false;
    struct Slot {
        bool joined = false;
        int device = 0;
        const double* ptr[2] = {nullptr, nullptr};          // the parity buffer published for the collective in flight
        const int64_t* send_off[2] = {nullptr, nullptr};    // exchange: the publisher's segment bounds (host array, stable while the plan lives); nullptr: an all-reduce
        hipEvent_t ready[2] = {nullptr, nullptr}, done[2] = {nullptr, nullptr};
        double* stage[2] = {nullptr, nullptr};               // all-reduce: copies of the operand
        size_t stage_cap[2] = {0, 0};
        void release() {
            for (int k = 0; k < 2; ++k) {
                if (ready[k]) (void)hipEventDestroy(ready[k]);
                if (done[k]) (void)hipEventDestroy(done[k]);
                if (stage[k]) (void)hipFree(stage[k]);
            }
            *this = Slot{};
        }
    } slot[MAX_RANKS];
    ~Group() { for (Slot& s : slot) s.release(); }      // what a rank destroyed without pgo_comm_destroy left behind

    // all ranks arrive or the group is broken (a rank failed / left, or nobody came for two minutes): false
    bool barrier() {
        std::unique_lock<std::mutex> lk(m);
        if (broken) return false;
        const uint64_t gen = generation;
        if (++arrived == world) { arrived = 0; ++generation; cv.notify_all(); return true; }
        const bool ok = cv.wait_for(lk, std::chrono::seconds(120), [&]() { return generation != gen || broken; });
        if (!ok) { broken = true; cv.notify_all(); return false; }
        return !broken || generation != gen;
    }
    void abort() { std::lock_guard<std::mutex> lk(m); broken = true; cv.notify_all(); }
};

// an error return once a collective (or the join) has begun releases the peers at once: their calls return PGO_ERR_COMM instead of waiting at the barrier for two minutes
struct AbortUnlessDone {
    Group* G;
    bool done = false;
    ~AbortUnlessDone() { if (!done) G->abort(); }
};

struct LocalComm final : Comm {
    LocalComm(Group* G, int rank, hipStream_t st) : Comm(rank, G->world, st), G(G) {}
    ~LocalComm() override {
        if (abandoned) { G->abort(); return; }      // (a peer's kernel may still read this slot's buffers: pgo_local_group_destroy frees them)
        // every rank's stream has drained before any event or staging buffer goes (a peer's kernel may still be reading them)
        (void)hipStreamSynchronize(st_);
        (void)G->barrier();
        G->slot[rank_].release();
    }
    // step 1: this collective's parity buffer may be overwritten once the peers' reads of it two collectives ago are done
    int send_slot(std::string& err) override {
        AbortUnlessDone guard{G};
        const int par = (int)(count & 1);
        for (int q = 0; q < world_; ++q) if (q != rank_ && G->slot[q].done[par]) HIPCHK(hipStreamWaitEvent(st_, G->slot[q].done[par], 0));
        guard.done = true;
        return par;
    }
    int allreduce(double* buf, size_t n, int op, std::string& err) override {
        const int rc = send_slot(err);
        if (rc < 0) return rc;
        return collective(buf, n, nullptr, "collective", err, [&](int par, pgo::LocalPeers& P) -> int {
            for (int q = 0; q < world_; ++q) {
                P.src[q] = G->slot[q].ptr[par]; P.off[q] = 0; P.cnt[q] = (int64_t)n;
                if (q != rank_) HIPCHK(hipStreamWaitEvent(st_, G->slot[q].ready[par], 0));
            }
            P.n = world_;
            pgo::launch_local_reduce(buf, P, (int64_t)n, op, st_);
            return PGO_OK;
        });
    }
    // `send` is the parity buffer of send_slot(), already packed
    int exchange(const ExchangeView& X, int K, const double* send, double* recv, std::string& err, size_t&) override {
        return collective(send, 0, X.send_off, "exchange", err, [&](int par, pgo::LocalPeers& P) -> int {
            for (int q = 0; q < world_; ++q) {
                const int64_t cnt = (X.recv_off[q + 1] - X.recv_off[q]) * K;
                if (q == rank_ || cnt == 0) continue;
                const int64_t* so = G->slot[q].send_off[par];
                if (!so || (so[rank_ + 1] - so[rank_]) * K != cnt) { err = "in-process communicator: the ranks' exchange plans disagree"; return PGO_ERR_COMM; }
                HIPCHK(hipStreamWaitEvent(st_, G->slot[q].ready[par], 0));
                P.src[P.n] = G->slot[q].ptr[par] + so[rank_] * K; P.off[P.n] = X.recv_off[q] * K; P.cnt[P.n] = cnt; ++P.n;
            }
            if (P.n > 0) pgo::launch_local_copy(recv, P, st_);
            return PGO_OK;
        });
    }
    bool barrier() override { return G->barrier(); }
    void abandon() override { abandoned = true; }
    // steps 2-4: publish `buf` (an all-reduce, without segment bounds: a staged copy of its `stage_n` doubles), meet the peers; `read` waits on the peers it reads, launches the kernel
    template <class Read>
    int collective(const double* buf, size_t stage_n, const int64_t* send_off, const char* what, std::string& err, Read read) {
        AbortUnlessDone guard{G};
        Group::Slot& me = G->slot[rank_];
        const int par = (int)(count & 1);
        int rc;
        if (send_off == nullptr) {
            if ((rc = grow(me.stage[par], me.stage_cap[par], stage_n, st_, err)) != PGO_OK) return rc;
            HIPCHK(hipMemcpyAsync(me.stage[par], buf, stage_n * sizeof(double), hipMemcpyDeviceToDevice, st_));
            buf = me.stage[par];
        }
        HIPCHK(hipEventRecord(me.ready[par], st_));
        me.ptr[par] = buf; me.send_off[par] = send_off;
        if (!G->barrier()) { err = std::string("in-process communicator: a rank did not reach the ") + what + " (failed, left, or out of step)"; return PGO_ERR_COMM; }
        pgo::LocalPeers P{};
        if ((rc = read(par, P)) != PGO_OK) return rc;
        HIPCHK(hipEventRecord(me.done[par], st_));
        ++count;
        guard.done = true;
        return PGO_OK;
    }
    Group* G;
    uint64_t count = 0;      // collectives issued so far (parity = count & 1)
    bool abandoned = false;
};

}  // namespace

int make_rccl_comm(const uint8_t id[PGO_COMM_ID_BYTES], int rank, int world, hipStream_t st, std::unique_ptr<Comm>& out, std::string& err) {
    std::unique_ptr<RcclComm> c(new RcclComm(rank, world, st));
    Rccl::Uid u;
    std::memcpy(u.b, id, PGO_COMM_ID_BYTES);
    int rc;
    if ((rc = load_rccl(c->R, err)) != PGO_OK) return rc;
    if ((rc = c->R.CommInitRank(&c->comm, world, u, rank)) != 0) { c->comm = nullptr; err = c->R.error("ncclCommInitRank", rc); return PGO_ERR_COMM; }
    out = std::move(c);
    return PGO_OK;
}
std::unique_ptr<Comm> make_custom_comm(pgo_allreduce_fn fn, void* ctx, int rank, int world, hipStream_t st) { return std::unique_ptr<Comm>(new CustomComm(fn, ctx, rank, world, st)); }
int make_local_comm(void* group, int rank, int world, int device, hipStream_t st, std::unique_ptr<Comm>& out, std::string& err) {
    Group* G = static_cast<Group*>(group);
    if (world != G->world) return PGO_ERR_INVALID_ARG;
    Group::Slot& me = G->slot[rank];
    if (me.joined) { err = "in-process communicator: the rank is taken"; return PGO_ERR_INVALID_ARG; }
    me.device = device; me.joined = true;
    out.reset(new LocalComm(G, rank, st));      // (from here on its destructor leaves the slot)
    AbortUnlessDone guard{G};
    for (int k = 0; k < 2; ++k) {
        HIPCHK(hipEventCreateWithFlags(&me.ready[k], hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&me.done[k], hipEventDisableTiming));
    }
    // ranks on other GPUs of this process: their buffers are read over xGMI (peer access); every rank has joined once all have passed this barrier
    if (!G->barrier()) { err = "in-process communicator: not all ranks joined"; return PGO_ERR_COMM; }
    for (int q = 0; q < world; ++q) {
        if (q == rank || G->slot[q].device == device) continue;
        const hipError_t e = hipDeviceEnablePeerAccess(G->slot[q].device, 0);
        (void)hipGetLastError();
        if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) { err = "in-process communicator: no peer access between the ranks' GPUs"; return PGO_ERR_COMM; }
    }
    guard.done = true;
    return PGO_OK;
}

}  // namespace pgo_comm

int pgo_comm_get_unique_id(uint8_t id[PGO_COMM_ID_BYTES]) {
    if (!id) return PGO_ERR_INVALID_ARG;
    std::string err;
    pgo_comm::Rccl::Uid u;
    if (pgo_comm::load_rccl(pgo_comm::g_rccl_for_id, err) != PGO_OK || pgo_comm::g_rccl_for_id.GetUniqueId(&u) != 0) return PGO_ERR_COMM;
    std::memcpy(id, u.b, PGO_COMM_ID_BYTES);
    return PGO_OK;
}
int pgo_local_group_create(int32_t world, void** group) {
    if (!group || world < 1 || world > pgo_comm::MAX_RANKS) return PGO_ERR_INVALID_ARG;
    pgo_comm::Group* G = new (std::nothrow) pgo_comm::Group();
    if (!G) return PGO_ERR_OUT_OF_MEMORY;
    G->world = world;
    *group = G;
    return PGO_OK;
}
int pgo_local_group_abort(void* group) {
    if (!group) return PGO_ERR_INVALID_ARG;
    static_cast<pgo_comm::Group*>(group)->abort();
    return PGO_OK;
}
int pgo_local_group_destroy(void* group) {
    if (!group) return PGO_ERR_INVALID_ARG;
    delete static_cast<pgo_comm::Group*>(group);
    return PGO_OK;
}
