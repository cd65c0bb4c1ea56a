// pgo_comm.hpp — the multi-rank transports of libpgo behind one interface: RCCL (pgo_comm_init), a caller-supplied collective (pgo_comm_init_custom, pgo_comm_set_exchange)
// and the in-process group (pgo_comm_init_local).  A handle holds at most one Comm and issues every collective through it; one GPU has none.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <string>

#include "pgo.h"

namespace pgo_comm {

// segment bounds of one neighbour exchange in rows (pgo_mg_host.hpp: ExchangePlan): send_off / recv_off [world + 1], pair_cnt [world * world] (src sends to dst at src * world + dst)
struct ExchangeView { const int64_t* send_off; const int64_t* recv_off; const int64_t* pair_cnt; };

// One transport, one lifetime: the destructor is the whole teardown.  Every call is enqueued on the stream the transport was made with; errors are PGO_ERR_* codes, text in `err`.
struct Comm {
    Comm(int rank, int world, hipStream_t st) : rank_(rank), world_(world), st_(st) {}
    virtual ~Comm() { if (scratch_) (void)hipFree(scratch_); }
    int rank() const { return rank_; }
    int world() const { return world_; }
    virtual int allreduce(double* buf, size_t n, int op /*0 sum, 2 max*/, std::string& err) = 0;
    // the send buffer (0 / 1) the exchange about to be packed fills, or an error: the in-process group double-buffers by collective parity and waits for the peers' reads of it
    virtual int send_slot(std::string&) { return 0; }
    // rows [send_off[q], send_off[q+1]) of `send` (K doubles each) go to rank q, rows [recv_off[q], recv_off[q+1]) of `recv` come from it; `reduced`: doubles all-reduced by an emulation
    virtual int exchange(const ExchangeView& X, int K, const double* send, double* recv, std::string& err, size_t& reduced) = 0;
    virtual bool barrier() { return true; }                        // pgo_time_kernel's turns: only ranks sharing a process meet
    virtual bool graph_capturable() const { return false; }        // a PCG chunk holding these collectives may be captured as a hipGraph
    virtual bool set_exchange(pgo_exchange_fn) { return false; }   // caller-supplied collective only
    virtual void abandon() {}                                      // the handle goes without pgo_comm_destroy: the peers may be gone, do not wait for them

protected:
    // the exchange as an all-reduce of a zero-padded buffer holding every pair's segment, through this transport's own all-reduce (world x the bytes)
    int exchange_via_allreduce(const ExchangeView& X, int K, const double* send, double* recv, std::string& err, size_t& reduced);
    const int rank_, world_;
    const hipStream_t st_;
    double* scratch_ = nullptr;
    size_t scratch_cap_ = 0;
};

int make_rccl_comm(const uint8_t id[PGO_COMM_ID_BYTES], int rank, int world, hipStream_t st, std::unique_ptr<Comm>& out, std::string& err);
std::unique_ptr<Comm> make_custom_comm(pgo_allreduce_fn fn, void* ctx, int rank, int world, hipStream_t st);
int make_local_comm(void* group, int rank, int world, int device, hipStream_t st, std::unique_ptr<Comm>& out, std::string& err);

}  // namespace pgo_comm
