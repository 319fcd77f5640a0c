// msx_engine.h — what the collective engine's translation units share.
//
// Internal to the files split out of the former single transport unit:
//   msx_transport.cpp    bootstrap hub, shared-memory barrier, uncached pool, IpcTransport
//   msx_schedule.cpp     the pure schedule functions (declared in msx_transport.h)
//   msx_engine.cpp       worker thread, window geometry, copies, user-op host path
//   msx_rccl.cpp         RCCL loader and both RCCL planes
//   msx_collectives.cpp  allreduce / reduce / reduce_scatter / scan schedules
//   msx_devop.cpp        the same collectives with a device-resident user op
//   msx_rma.cpp          fence, passive-target and PSCW one-sided operations
//   msx_intercomm.cpp    world mailbox, intercommunicators, communicator split / free
// Never included by an entry-point unit (msx_api.cpp, msx_api_reduce.cpp,
// msx_api_request.cpp, msx_api_rma.cpp, msx_api_ext.cpp), msx_comm.cpp or a
// .hip unit: they see the
// engine through msx_transport.h only.  Every piece of state named here has
// its one definition in the .cpp that owns it.
//
// Reference anchors (src/mpi/msmpi/mpid/reduce.cpp):
//   MPIR_Allreduce_intra_flat            :3768-4104  (fold, RD / Rabenseifner, unfold)
//   MPIR_Reduce_scatter_intra_impl       :1636-1770  (algorithm gate, 32-bit nbytes)
//   MPIR_Reduce_scatter_commutative_short:917-1219   (recursive halving)
//   MPIR_Reduce_scatter_commutative_long :1225-1334  (pairwise exchange)
// The reference moves partial results between ranks step by step
// (MPIC_Sendrecv) and combines after each step (MPID_Uop_call).  Here each
// rank reads every contribution it needs straight from its peers' HBM and
// evaluates the SAME expression tree (same association, same inout/in roles)
// in one kernel, so results are bit-identical to the reference schedule.
#pragma once

#include "msx_transport.h"   // first: <hip/hip_runtime.h> before the C++ library headers, as in every unit

#include <condition_variable>
#include <deque>
#include <functional>
#include <future>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "msx_dtype.h"
#include "msx_kernels.h"
#include "msx_runtime.h"

// RCCL's communicator handle, opaque here: only msx_rccl.cpp includes <rccl/rccl.h>
struct ncclComm;
typedef struct ncclComm* ncclComm_t;

namespace msx {

// ---- msx_transport.cpp ------------------------------------------------------
double now_s();

// ---- msx_engine.cpp ---------------------------------------------------------
// Collectives on one communicator run in issue order on one worker thread,
// so blocking and non-blocking calls share the hub in the order every rank
// issued them (MPI requires the same order on all ranks).
class Worker {
public:
    ~Worker()
    {
        {
            std::lock_guard<std::mutex> g(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        if (th_.joinable()) th_.join();
    }
    std::shared_future<int> submit(std::function<int()> fn)
    {
        if (std::this_thread::get_id() == tid_) {
            // re-entrant call from a collective already on the worker: run inline
            std::promise<int> pr;
            pr.set_value(fn());
            return pr.get_future().share();
        }
        auto task = std::make_shared<std::packaged_task<int()>>(std::move(fn));
        std::shared_future<int> f = task->get_future().share();
        {
            std::lock_guard<std::mutex> g(mu_);
            if (!th_.joinable()) {
                th_ = std::thread([this] { loop(); });
                tid_ = th_.get_id();
            }
            q_.push_back(task);
        }
        cv_.notify_all();
        return f;
    }

    // A blocking call: run it on the calling thread when the worker is idle
    // (no queued or running task -- the collective order is then the issue
    // order anyway), which saves two thread hand-offs (~10-20 us) per call;
    // otherwise queue it behind the pending non-blocking operations.
    int run(std::function<int()> fn)
    {
        if (std::this_thread::get_id() == tid_) return fn();
        {
            std::unique_lock<std::mutex> g(mu_);
            if (!q_.empty() || busy_ || inline_) {
                g.unlock();
                // the error text is thread-local: carry it back to the caller
                auto text = std::make_shared<std::string>();
                const int rc = submit([fn = std::move(fn), text]() -> int {
                                   const int r = fn();
                                   if (r != MPI_SUCCESS) *text = last_error();
                                   return r;
                               }).get();
                if (rc != MPI_SUCCESS) set_error("%s", text->c_str());
                return rc;
            }
            inline_ = true;
        }
        const int rc = fn();
        {
            std::lock_guard<std::mutex> g(mu_);
            inline_ = false;
        }
        cv_.notify_all();
        return rc;
    }

private:
    void loop()
    {
        // a new thread starts on HIP device 0: bind it to this rank's GPU
        // before any task allocates (one rank per GPU on a multi-GPU node)
        (void)ensure_device();
        for (;;) {
            std::shared_ptr<std::packaged_task<int()>> t;
            {
                std::unique_lock<std::mutex> g(mu_);
                cv_.wait(g, [this] { return stop_ || (!q_.empty() && !inline_); });
                if (q_.empty()) return;
                t = q_.front();
                q_.pop_front();
                busy_ = true;
            }
            (*t)();
            std::lock_guard<std::mutex> g(mu_);
            busy_ = false;
        }
    }
    std::mutex mu_;
    std::condition_variable cv_;
    std::deque<std::shared_ptr<std::packaged_task<int()>>> q_;
    std::thread th_;
    std::thread::id tid_;
    bool stop_ = false;
    bool busy_ = false;     // the worker is running a task
    bool inline_ = false;   // a blocking call runs on its caller's thread
};

Worker& worker();

int flag_timeout(const char* op, int me, int word, unsigned long long seq, bool index_is_rank = true);
bool fault_drop_flags(int me, unsigned long long seq);
int sync_stream(hipStream_t s, const char* what);

// What run_rank_tree's launch posts when it ends (the two-step allreduce)
struct TreeWait {
    // result-ready flags after the last of `done_launches` launches
    // (TreeSpec::done_*); done_counter: block 2 of push_counter()
    unsigned* done_counter = nullptr;
    unsigned done_launches = 1;
    const std::vector<unsigned long long*>* done_flags = nullptr;
    unsigned long long done_seq = 0;
};

int run_rank_tree(int opidx, Kind k, const RankTree& t, const std::vector<char*>& srcs, size_t esz,
                  size_t start, size_t len, char* out, hipStream_t s,
                  const std::vector<char*>& extra_outs = {}, const TreeWait* wait = nullptr);

// host path for user-defined ops: the image of `count` elements of a datatype
struct Img {
    int64_t lo = 0;            // image byte 0 = typed byte lo
    size_t bytes = 0;
    const Dtype* t = nullptr;  // derived type, or null (predefined)
    size_t esz = 0;            // predefined element size
};

Img img_of(MPI_Datatype dt, size_t count);
int img_load(const Img& m, const void* buf, char* img);
int img_store(const Img& m, size_t count, const char* typed_base, void* buf);
void img_call(const OpRef& op, MPI_Datatype dt, const Img& m, size_t count, const char* in, char* io);
int host_user_run(Comm* c, const void* src, void* recvbuf, size_t total, MPI_Datatype dt, const OpRef& op,
                  const CombinePlan* plan, size_t first, size_t count, size_t out_first, size_t out_count);
int host_user_allreduce(Comm* c, const void* sendbuf, void* recvbuf, size_t count,
                        MPI_Datatype dt, const OpRef& op);

char* dev_scratch(size_t bytes);
size_t chunk_bytes();
size_t rma_bytes_for(int share);   // passive-target staging size for `share` ranks per GPU
size_t sub_skew(size_t per_rank);
size_t sub_len(size_t C, int p);
size_t half_bytes(int p);          // one half of an IN sub-slot (the GPU-flag schedules' unit)

// Every rank's engine window as this process maps it (layout: msx_engine.cpp,
// "window collectives")
struct Windows {
    std::vector<char*> base;
    size_t C = 0, Q = 0, S = 0, I = 0;   // chunk, sub-slot length, sub-slot stride, IN area bytes
    char* in(int r) const { return base[(size_t)r]; }
    char* sub(int r, int k) const { return base[(size_t)r] + (size_t)k * S; }
    char* out(int r) const { return base[(size_t)r] + I; }
    unsigned long long* flags(int r) const { return reinterpret_cast<unsigned long long*>(base[(size_t)r] + I + C); }
    // passive-target staging (rma_window), when the communicator has one
    std::vector<char*> rbase;
    size_t rbytes = 0;                    // the agreed staging size (rma_window)
    size_t rma_slot() const { return (rbytes / (2 * rbase.size())) & ~(size_t)255; }
    // rank r's staging: payload slot written by origin o / fetch slot written by target t
    char* rma_in(int r, int o) const { return rbase[(size_t)r] + (size_t)o * rma_slot(); }
    char* rma_fetch(int r, int t) const { return rbase[(size_t)r] + (rbase.size() + (size_t)t) * rma_slot(); }
};

// Result-ready flags of the two-step allreduce live in the upper half of the
// flag area: slot kResultFlags + k of window r = the last call whose result
// rank k stored into r's OUT area.
constexpr size_t kResultFlags = 4096;
// Scan partials' arrival flags: slot kScanFlags + k of window r = (call << 6)
// | step of the last partial rank k pushed to r (only scan writes them).
constexpr size_t kScanFlags = 2048;
// GPU "done" flags of the pipelined two-step allreduce: slot kDoneFlags + k of
// window r = the last chunk (flag sequence number) whose IN / OUT halves rank
// k finished reading; a chunk two later may then overwrite them.
constexpr size_t kDoneFlags = 6144;

size_t two_step_max(const Transport* tp);
Bounce& engine_bounce(int i);
int* wait_err_word(int** host);
int get_windows(Transport* tp, Windows* w, bool rd_single = false);
int copy_async(void* dst, const void* src, size_t bytes, hipStream_t s);

// Phase timers of the window allreduce (host clock, engine worker only):
// t[0] stage + scatter, t[1] collect wait + barrier A, t[2] reduce + push,
// t[3] barrier B, t[4] last collect.  Read by msx_engine_stats().
struct EngineStats {
    double t[5] = {0, 0, 0, 0, 0};
    long chunks = 0, calls = 0;
    long flag_calls = 0;   // GPU-flag Rabenseifner calls (two-step allreduce / reduce, flag reduce_scatter)
};
extern EngineStats g_stats;

hipStream_t aux_stream(Transport* tp);

// A batch of byte ranges moved by one k_copy_segs launch (one grid row each).
struct Segs {
    std::vector<const void*> src;
    std::vector<void*> dst;
    std::vector<size_t> n;
    void add(const void* s, void* d, size_t bytes)
    {
        if (!bytes) return;
        src.push_back(s);
        dst.push_back(d);
        n.push_back(bytes);
    }
    int run(hipStream_t s, const char* what)
    {
        if (src.empty()) return MPI_SUCCESS;
        hipError_t e = launch_copy_segs(src.data(), dst.data(), n.data(), (int)src.size(), s);
        return e == hipSuccess ? MPI_SUCCESS : hip_fail(e, what);
    }
};

int device_view(const BufInfo& b, const char* user, size_t off, size_t len, char* stage,
                hipStream_t s, const char** out);

// ---- msx_rccl.cpp -----------------------------------------------------------
bool rccl_requested();
bool rccl_native_requested();
void rccl_forget(Transport* tp);   // the RCCL plane's per-transport state
ncclComm_t rccl_comm(Transport* tp);
int rccl_allreduce(ncclComm_t comm, Comm* c, const void* sendbuf, void* recvbuf, size_t count,
                   MPI_Datatype dt, const OpRef& op, int root, bool nbc);
int rccl_reduce_scatter(ncclComm_t comm, Comm* c, const void* sendbuf, void* recvbuf, const int* recvcounts,
                        MPI_Datatype dt, const OpRef& op);

// ---- msx_collectives.cpp ----------------------------------------------------
int do_allreduce(Comm* c, const void* sendbuf, void* recvbuf, size_t count, MPI_Datatype dt,
                 const OpRef& op, int root = -1, bool nbc = false);
int host_user_reduce(Comm* c, const void* sendbuf, void* recvbuf, size_t count, MPI_Datatype dt,
                     const OpRef& op, int root);

// ---- msx_devop.cpp ----------------------------------------------------------
// The reduction collectives with a device user op (op.dev_fn): a device gather
// over the windows, then the host user-op path's order evaluated in device
// scratch with the user's launches.  Engine worker (or the inline blocking call).
int devop_allreduce(Comm* c, const void* sendbuf, void* recvbuf, size_t count, MPI_Datatype dt, const OpRef& op);
int devop_reduce(Comm* c, const void* sendbuf, void* recvbuf, size_t count, MPI_Datatype dt, const OpRef& op,
                 int root);
int devop_reduce_scatter(Comm* c, const void* sendbuf, void* recvbuf, const int* recvcounts, MPI_Datatype dt,
                         const OpRef& op);
int devop_scan(Comm* c, const void* sendbuf, void* recvbuf, size_t count, MPI_Datatype dt, const OpRef& op,
               bool exclusive);

// ---- msx_rma.cpp ------------------------------------------------------------
void futex_wake_all(void* addr);
void futex_wait_ms(void* addr, uint32_t val, long ms);
int shm_collective(Transport* tp, size_t bytes, void** out);

// ---- msx_intercomm.cpp (for engine_intercomm_create, which needs IpcTransport
// and so lives in msx_transport.cpp) ------------------------------------------
int mail_send(int dst, int tag, const void* data, size_t n);
int mail_recv(int src, int tag, std::vector<char>* out);
int group_bcast(Comm* c, std::vector<int32_t>& v, int root);
int dup_intra(Comm* c, Comm** out);
void free_intra(Comm* c);
int map_union(Comm* u);

}  // namespace msx
