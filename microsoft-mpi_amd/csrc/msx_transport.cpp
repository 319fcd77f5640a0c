// msx_transport.cpp — bootstrap hub, shared-memory barrier, uncached-memory
// pool and the IPC transport (peer mapping, engine and RMA windows).
//
// The schedules and the engine that runs over a Transport live in
// msx_schedule.cpp, msx_engine.cpp, msx_rccl.cpp, msx_collectives.cpp,
// msx_rma.cpp and msx_intercomm.cpp (msx_engine.h has the map).
#include "msx_transport.h"

#include <arpa/inet.h>
#include <algorithm>
#include <atomic>
#include <errno.h>
#include <fcntl.h>
#include <linux/futex.h>
#include <map>
#include <mutex>
#include <netdb.h>
#include <netinet/in.h>
#include <netinet/tcp.h>
#include <poll.h>
#include <sched.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <sys/mman.h>
#include <sys/socket.h>
#include <sys/syscall.h>
#include <time.h>
#include <unistd.h>

#include "msx_engine.h"
#include "msx_kernels.h"
#include "msx_runtime.h"

namespace msx {

// ===========================================================================
// bootstrap hub: rank 0 listens, every other rank keeps one TCP connection
// ===========================================================================
double now_s()
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec + ts.tv_nsec * 1e-9;
}

namespace {

int io_all(int fd, void* buf, size_t n, bool wr, double timeout_s)
{
    char* p = static_cast<char*>(buf);
    const double t_end = now_s() + timeout_s;
    while (n) {
        struct pollfd pf = {fd, (short)(wr ? POLLOUT : POLLIN), 0};
        int ms = (int)((t_end - now_s()) * 1000);
        if (ms <= 0) { set_error("bootstrap: timed out"); return MPI_ERR_OTHER; }
        int pr = poll(&pf, 1, ms < 1000 ? ms : 1000);
        if (pr < 0 && errno == EINTR) continue;
        if (pr < 0) { set_error("bootstrap poll: %s", strerror(errno)); return MPI_ERR_OTHER; }
        if (pr == 0) continue;
        ssize_t k = wr ? send(fd, p, n, MSG_NOSIGNAL) : recv(fd, p, n, 0);
        if (k < 0 && (errno == EINTR || errno == EAGAIN)) continue;
        if (k <= 0) { set_error("bootstrap: peer connection lost (%s)", k ? strerror(errno) : "eof"); return MPI_ERR_OTHER; }
        p += k;
        n -= (size_t)k;
    }
    return MPI_SUCCESS;
}

class Hub {
public:
    ~Hub()
    {
        for (int fd : fd_) if (fd >= 0) close(fd);
        if (lfd_ >= 0) close(lfd_);
    }

    // MPI_COMM_WORLD: the hub address from the launcher's environment
    int init(int rank, int size)
    {
        const char* addr = getenv("MSX_BOOTSTRAP_ADDR");
        if (!addr) addr = getenv("MASTER_ADDR");
        if (!addr) addr = "127.0.0.1";
        int port = 29571;
        if (const char* v = getenv("MSX_BOOTSTRAP_PORT")) port = atoi(v);
        else if (const char* v = getenv("MASTER_PORT")) port = (atoi(v) + 97) % 65536;
        if (port < 1024) port += 1024;
        return init_at(rank, size, addr, port, -1);
    }

    // A derived communicator: its rank 0 already listens on `lfd` (bound to
    // an ephemeral port published through the parent); the others connect.
    int init_at(int rank, int size, const char* addr, int port, int lfd)
    {
        rank_ = rank;
        size_ = size;
        timeout_ = 600.0;
        if (const char* t = getenv("MSX_BOOTSTRAP_TIMEOUT")) timeout_ = atof(t);

        struct addrinfo hints = {}, *res = nullptr;
        hints.ai_family = AF_INET;
        hints.ai_socktype = SOCK_STREAM;
        char ps[16];
        snprintf(ps, sizeof(ps), "%d", port);
        if (getaddrinfo(addr, ps, &hints, &res) != 0 || !res) {
            set_error("bootstrap: cannot resolve %s", addr);
            return MPI_ERR_OTHER;
        }
        struct sockaddr_in sa;
        memcpy(&sa, res->ai_addr, sizeof(sa));
        freeaddrinfo(res);
        fd_.assign((size_t)size, -1);

        if (rank == 0) {
            int one = 1;
            if (lfd >= 0) {
                lfd_ = lfd;
            } else {
                lfd_ = socket(AF_INET, SOCK_STREAM, 0);
                setsockopt(lfd_, SOL_SOCKET, SO_REUSEADDR, &one, sizeof(one));
                struct sockaddr_in any = sa;
                if (bind(lfd_, (struct sockaddr*)&any, sizeof(any)) != 0) {
                    set_error("bootstrap: bind %s:%d: %s", addr, port, strerror(errno));
                    return MPI_ERR_OTHER;
                }
                listen(lfd_, size + 8);
            }
            const double t_end = now_s() + timeout_;
            for (int got = 1; got < size;) {
                struct pollfd pf = {lfd_, POLLIN, 0};
                int ms = (int)((t_end - now_s()) * 1000);
                if (ms <= 0) { set_error("bootstrap: only %d of %d ranks connected", got, size); return MPI_ERR_OTHER; }
                if (poll(&pf, 1, ms) <= 0) continue;
                int fd = accept(lfd_, nullptr, nullptr);
                if (fd < 0) continue;
                setsockopt(fd, IPPROTO_TCP, TCP_NODELAY, &one, sizeof(one));
                int32_t r = -1;
                if (io_all(fd, &r, 4, false, timeout_) != MPI_SUCCESS || r <= 0 || r >= size || fd_[r] >= 0) {
                    close(fd);
                    continue;
                }
                fd_[r] = fd;
                ++got;
            }
        } else {
            const double t_end = now_s() + timeout_;
            int fd = -1;
            while (true) {
                fd = socket(AF_INET, SOCK_STREAM, 0);
                if (connect(fd, (struct sockaddr*)&sa, sizeof(sa)) == 0) break;
                close(fd);
                fd = -1;
                if (now_s() > t_end) { set_error("bootstrap: cannot reach rank 0 at %s:%d", addr, port); return MPI_ERR_OTHER; }
                usleep(20000);
            }
            int one = 1;
            setsockopt(fd, IPPROTO_TCP, TCP_NODELAY, &one, sizeof(one));
            int32_t r = rank;
            if (io_all(fd, &r, 4, true, timeout_) != MPI_SUCCESS) { close(fd); return MPI_ERR_OTHER; }
            fd_[0] = fd;
        }
        return MPI_SUCCESS;
    }

    // Every rank contributes n bytes; all receive size*n bytes in rank order.
    int allgather(const void* mine, size_t n, void* all)
    {
        std::lock_guard<std::mutex> g(mu_);
        char* out = static_cast<char*>(all);
        auto fail = [&](int peer, const char* phase) {
            const std::string why = last_error();
            set_error("wait timeout: op=hub_allgather rank=%d phase=%s peer=%d limit_s=%.1f (%s)", rank_, phase, peer,
                      timeout_, why.c_str());
            return MPI_ERR_OTHER;
        };
        if (rank_ == 0) {
            memcpy(out, mine, n);
            for (int r = 1; r < size_; ++r)
                if (io_all(fd_[r], out + (size_t)r * n, n, false, timeout_) != MPI_SUCCESS) return fail(r, "gather");
            for (int r = 1; r < size_; ++r)
                if (io_all(fd_[r], out, (size_t)size_ * n, true, timeout_) != MPI_SUCCESS) return fail(r, "scatter");
            return MPI_SUCCESS;
        }
        if (io_all(fd_[0], const_cast<void*>(mine), n, true, timeout_) != MPI_SUCCESS) return fail(0, "send");
        if (io_all(fd_[0], out, (size_t)size_ * n, false, timeout_) != MPI_SUCCESS) return fail(0, "receive");
        return MPI_SUCCESS;
    }

private:
    int rank_ = 0, size_ = 1, lfd_ = -1;
    double timeout_ = 600.0;
    std::vector<int> fd_;
    std::mutex mu_;
};

// ===========================================================================
// node-local barrier in POSIX shared memory (all ranks of a communicator are
// on one node: the IPC engine requires it).  Sense-reversing counter: a few
// microseconds instead of a TCP round trip through the hub.
// ===========================================================================
constexpr int kDoneSlots = 480;
struct ShmBar {
    std::atomic<uint32_t> count;
    std::atomic<uint32_t> gen;
    // per rank: sequence number of the last barrier-free call it has finished
    // (its tree has read its IN half), see do_allreduce
    std::atomic<uint64_t> done[kDoneSlots];
    // per rank: 1 + the generation of the barrier it last entered (timeouts
    // name the ranks that never arrived)
    std::atomic<uint32_t> at[kDoneSlots];
};
constexpr size_t kShmBarBytes = 8192;
static_assert(sizeof(ShmBar) <= kShmBarBytes, "two pages");

class ShmBarrier {
public:
    ~ShmBarrier()
    {
        if (bar_) munmap(bar_, kShmBarBytes);
    }

    // Collective over the hub.  Returns false (and stays unused) when shared
    // memory is unavailable; the caller then keeps the hub barrier.
    bool init(Hub& hub, int rank, int size, double timeout_s)
    {
        size_ = size;
        rank_ = rank;
        timeout_ = timeout_s;
        char name[64] = {0};
        int fd = -1;
        if (rank == 0) {
            // created and sized before anyone learns the name
            snprintf(name, sizeof(name), "/msx_bar_%d_%ld", (int)getpid(), (long)(now_s() * 1e6));
            fd = shm_open(name, O_CREAT | O_RDWR, 0600);
            if (fd < 0 || ftruncate(fd, kShmBarBytes) != 0) name[0] = 0;
        }
        std::vector<char> all((size_t)size * sizeof(name));
        if (hub.allgather(name, sizeof(name), all.data()) != MPI_SUCCESS) {
            if (fd >= 0) close(fd);
            return false;
        }
        memcpy(name, all.data(), sizeof(name));
        int ok = name[0] != 0;
        if (ok && rank != 0) fd = shm_open(name, O_RDWR, 0600);
        std::vector<int> oks((size_t)size);
        void* m = MAP_FAILED;
        if (ok && fd >= 0) m = mmap(nullptr, kShmBarBytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
        if (fd >= 0) close(fd);
        int mine = (m != MAP_FAILED) ? 1 : 0;
        if (hub.allgather(&mine, sizeof(int), oks.data()) != MPI_SUCCESS) mine = 0;
        bool all_ok = mine != 0;
        for (int v : oks) all_ok = all_ok && v;
        if (rank == 0) shm_unlink(name);
        if (!all_ok) {
            if (m != MAP_FAILED) munmap(m, kShmBarBytes);
            trace("shm barrier unavailable; hub barrier in use");
            return false;
        }
        bar_ = static_cast<ShmBar*>(m);    // zero-filled by ftruncate
        return true;
    }

    bool ready() const { return bar_ != nullptr; }
    bool has_done() const { return bar_ && size_ <= kDoneSlots; }
    void post_done(int rank, uint64_t v) { bar_->done[rank].store(v, std::memory_order_release); }
    int wait_done(int rank, uint64_t v)
    {
        const double t_end = now_s() + timeout_;
        for (int spin = 0; bar_->done[rank].load(std::memory_order_acquire) < v; ++spin) {
            if (now_s() > t_end) {
                set_error("wait timeout: op=flag_call rank=%d phase=previous_call_done peer=%d seq=%llu limit_s=%.1f",
                          rank_, rank, (unsigned long long)v, timeout_);
                return MPI_ERR_OTHER;
            }
            if (spin > 2000) sched_yield();
        }
        return MPI_SUCCESS;
    }

    int wait()
    {
        const uint32_t g = bar_->gen.load(std::memory_order_acquire);
        if (size_ <= kDoneSlots) bar_->at[rank_].store(g + 1, std::memory_order_relaxed);
        if (bar_->count.fetch_add(1, std::memory_order_acq_rel) + 1 == (uint32_t)size_) {
            bar_->count.store(0, std::memory_order_relaxed);
            bar_->gen.store(g + 1, std::memory_order_release);
            syscall(SYS_futex, reinterpret_cast<uint32_t*>(&bar_->gen), FUTEX_WAKE, INT32_MAX, nullptr, nullptr, 0);
            return MPI_SUCCESS;
        }
        // short spin (the common case when ranks arrive together), then sleep
        // in the kernel on the generation word
        for (int it = 0; it < 4000; ++it)
            if (bar_->gen.load(std::memory_order_acquire) != g) return MPI_SUCCESS;
        const double t_end = now_s() + timeout_;
        while (bar_->gen.load(std::memory_order_acquire) == g) {
            if (now_s() > t_end) {
                // the first rank that has not entered this barrier
                int missing = -1;
                for (int r = 0; r < size_ && r < kDoneSlots && missing < 0; ++r)
                    if (bar_->at[r].load(std::memory_order_relaxed) != g + 1) missing = r;
                set_error("wait timeout: op=barrier rank=%d phase=host_barrier peer=%d seq=%u limit_s=%.1f", rank_,
                          missing, g, timeout_);
                return MPI_ERR_OTHER;
            }
            struct timespec ts = {0, 100 * 1000 * 1000};
            syscall(SYS_futex, reinterpret_cast<uint32_t*>(&bar_->gen), FUTEX_WAIT, g, &ts, nullptr, 0);
        }
        return MPI_SUCCESS;
    }

private:
    ShmBar* bar_ = nullptr;
    int size_ = 1;
    int rank_ = 0;
    double timeout_ = 600.0;
};

// ===========================================================================
// Uncached device memory: taken from the driver, never given back
// ===========================================================================
// Engine windows and RMA staging areas are uncached device memory
// (hipDeviceMallocUncached) that the peers map over IPC.  hipFree of such
// memory leaves this ROCm stack returning wrong data to later allocations'
// kernels and copies in the same process: after uncached buffers were used and
// freed, torch.equal(a, a.clone()) on fresh tensors failed in 4-30 of 96 cases
// per variant and a kernel write + copy check of a fresh plain buffer in 3 of
// 32; with the uncached buffers kept, 0 of 192 and 0 of 32; plain buffers or
// page-locked host memory freed the same way, 0 (scripts/va_reuse_probe.py,
// profiles/r06/va_reuse/).  So a freed communicator's window returns to this
// pool and serves the next window of the process (best fit), and imported peer
// windows stay mapped (ipc_imports); creating and freeing communicators then
// also costs no further 2 GiB allocations.
struct UcPool {
    struct Block {
        void* p;
        size_t cap;
        bool used;
    };
    std::mutex mu;
    std::vector<Block> blocks;
};

UcPool& uc_pool()
{
    static UcPool* pool = new UcPool();   // outlives static destruction: nothing is freed at exit either
    return *pool;
}

// `bytes` of zeroed uncached device memory on the current device.
hipError_t uc_alloc(size_t bytes, void** out)
{
    UcPool& pool = uc_pool();
    std::lock_guard<std::mutex> g(pool.mu);
    int dev = 0;
    (void)hipGetDevice(&dev);
    UcPool::Block* best = nullptr;
    for (auto& b : pool.blocks) {
        hipPointerAttribute_t a;
        if (b.used || b.cap < bytes || (best && b.cap >= best->cap)) continue;
        if (hipPointerGetAttributes(&a, b.p) != hipSuccess || a.device != dev) {
            (void)hipGetLastError();
            continue;
        }
        best = &b;
    }
    void* p = nullptr;
    if (best) {
        p = best->p;
    } else {
        hipError_t e = hipExtMallocWithFlags(&p, bytes, hipDeviceMallocUncached);
        if (e != hipSuccess) return e;
        pool.blocks.push_back({p, bytes, false});
        best = &pool.blocks.back();
    }
    hipError_t e = hipMemset(p, 0, bytes);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return e;
    best->used = true;
    *out = p;
    return hipSuccess;
}

void uc_release(void* p)
{
    if (!p) return;
    UcPool& pool = uc_pool();
    std::lock_guard<std::mutex> g(pool.mu);
    for (auto& b : pool.blocks)
        if (b.p == p) b.used = false;
}

// Peer windows imported over IPC, by handle, for the life of the process (an
// imported window is uncached memory too; closing the mapping is the same
// release as a free).  The exporter never frees a window (uc_pool), so a
// handle keeps naming the same memory.
struct IpcImports {
    std::mutex mu;
    std::map<std::string, void*> opened;
};

IpcImports& ipc_imports()
{
    static IpcImports* m = new IpcImports();
    return *m;
}

// ===========================================================================
// IPC transport
// ===========================================================================
struct IpcRec {
    hipIpcMemHandle_t h;
    uint64_t offset;
    int32_t ok;
    int32_t pad;
};

class IpcTransport : public Transport {
public:
    ~IpcTransport() override
    {
        uc_release(win_);    // windows go back to the pool, imports stay mapped (uc_pool)
        uc_release(rwin_);
        if (counter_) (void)hipFree(counter_);
        if (stream_) (void)hipStreamDestroy(stream_);
    }

    int init(int r, int s, int port = 0, int lfd = -1)
    {
        rank = r;
        size = s;
        int rc = port ? hub_.init_at(r, s, "127.0.0.1", port, lfd) : hub_.init(r, s);
        if (rc != MPI_SUCCESS) return rc;
        double t = 600.0;
        if (const char* v = getenv("MSX_BOOTSTRAP_TIMEOUT")) t = atof(v);
        (void)shm_.init(hub_, r, s, t);   // without it: the hub's barriers, no GPU-flag schedules
        // ranks that share a GPU (an unknown bus id shares nothing)
        char bus[32] = {0};
        int dev = -1;
        if (device_count_noinit() <= 0 || hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetPCIBusId(bus, sizeof(bus), dev) != hipSuccess) {
            (void)hipGetLastError();
            bus[0] = 0;
        }
        std::vector<char> buses((size_t)s * sizeof(bus));
        if ((rc = hub_.allgather(bus, sizeof(bus), buses.data())) != MPI_SUCCESS) return rc;
        for (int a = 0; a < s && !gpu_shared; ++a)
            for (int b = 0; b < a && !gpu_shared; ++b)
                gpu_shared = buses[(size_t)a * sizeof(bus)] != 0 &&
                             strncmp(buses.data() + (size_t)a * sizeof(bus), buses.data() + (size_t)b * sizeof(bus),
                                     sizeof(bus)) == 0;
        trace("transport: %d ranks, %s", s, gpu_shared ? "some share a GPU" : "one GPU each");
        return MPI_SUCCESS;
    }

    int allgather(const void* mine, size_t n, void* all) override { return hub_.allgather(mine, n, all); }

    bool has_done() const override { return shm_.has_done(); }
    void post_done(uint64_t v) override { shm_.post_done(rank, v); }
    int wait_done(int r, uint64_t v) override { return shm_.wait_done(r, v); }

    int barrier() override
    {
        if (shm_.ready()) return shm_.wait();
        char b = 0;
        std::vector<char> all((size_t)size);
        return hub_.allgather(&b, 1, all.data());
    }

    hipStream_t stream() override
    {
        if (!stream_) (void)hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking);
        return stream_;
    }

    unsigned* push_counter() override
    {
        if (!counter_) {
            // kCountBlocks blocks of kCountWords (msx_kernels.h)
            void* c = nullptr;
            const size_t bytes = (size_t)kCountBlocks * kCountWords * sizeof(unsigned);
            if (hipMalloc(&c, bytes) != hipSuccess) return nullptr;
            if (hipMemset(c, 0, bytes) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
                (void)hipFree(c);
                return nullptr;
            }
            counter_ = static_cast<unsigned*>(c);
        }
        return counter_;
    }

    int map_peers(const void* ptr, std::vector<char*>& out) override
    {
        IpcRec mine;
        memset(&mine, 0, sizeof(mine));
        void* base = nullptr;
        size_t asz = 0;
        hipError_t e = hipMemGetAddressRange(&base, &asz, const_cast<void*>(ptr));
        trace("map_peers: ptr=%p base=%p size=%zu rc=%d", ptr, base, asz, (int)e);
        if (e == hipSuccess) {
            PhaseScope ph("ipc_get_handle");
            e = hipIpcGetMemHandle(&mine.h, base);
        }
        trace("map_peers: handle rc=%d", (int)e);
        if (e == hipSuccess) {
            mine.ok = 1;
            mine.offset = (uint64_t)((const char*)ptr - (const char*)base);
        } else {
            (void)hipGetLastError();
            set_error("rank %d: buffer %p cannot be shared over IPC (%s)", rank, ptr, hipGetErrorString(e));
        }
        std::vector<IpcRec> all((size_t)size);
        int rc;
        {
            PhaseScope ph("ipc_handle_exchange");
            rc = hub_.allgather(&mine, sizeof(mine), all.data());
        }
        trace("map_peers: exchanged rc=%d", rc);
        if (rc != MPI_SUCCESS) return rc;
        out.assign((size_t)size, nullptr);
        for (int r = 0; r < size; ++r) {
            if (!all[r].ok) {
                if (r != rank) set_error("rank %d's buffer cannot be shared over IPC", r);
                return MPI_ERR_OTHER;
            }
            if (r == rank) { out[r] = const_cast<char*>(static_cast<const char*>(ptr)); continue; }
            std::string key(reinterpret_cast<const char*>(&all[r].h), sizeof(hipIpcMemHandle_t));
            IpcImports& imp = ipc_imports();
            std::lock_guard<std::mutex> g(imp.mu);
            auto it = imp.opened.find(key);
            void* pbase = nullptr;
            if (it != imp.opened.end()) {
                pbase = it->second;
            } else {
                {
                    PhaseScope ph("ipc_open", r);
                    e = hipIpcOpenMemHandle(&pbase, all[r].h, hipIpcMemLazyEnablePeerAccess);
                }
                trace("map_peers: opened rank %d handle -> %p rc=%d", r, pbase, (int)e);
                if (e != hipSuccess) {
                    hip_fail(e, "hipIpcOpenMemHandle");
                    set_error("ipc error: op=map_peers rank=%d phase=ipc_open peer=%d (%s)", rank, r, hipGetErrorString(e));
                    return MPI_ERR_OTHER;
                }
                imp.opened[key] = pbase;
            }
            out[r] = static_cast<char*>(pbase) + all[r].offset;
        }
        return MPI_SUCCESS;
    }

    int window(size_t bytes, std::vector<char*>& out) override
    {
        // Collective: every rank asks for the same size.
        if (bytes > win_bytes_) {
            uc_release(win_);
            win_ = nullptr;
            size_t want = bytes < ((size_t)1 << 20) ? ((size_t)1 << 20) : bytes;
            // Uncached device memory: peers write it over xGMI, which does not
            // snoop this GPU's L2, so no reader (kernel, blit or DMA) may hold a
            // stale line of it.  The kernel driver maps such a buffer MTYPE_UC
            // on the owner and on every peer that imports it, so neither the
            // writer's nor the reader's L2 ever holds a line of it, and the
            // engine's kernels need no per-workgroup system fences (each one
            // writes back or invalidates a whole XCD L2; rounds 1-2 had them and
            // they halved the collectives' throughput: p = 2 reduce_scatter
            // 4.17 -> 2.17 ms, allreduce 64 MiB 511 -> 178 us without).
            // zeroed (uc_alloc) before any peer can map it (map_peers below is
            // collective): the arrival flags behind the data areas start at 0
            hipError_t e = uc_alloc(want, &win_);
            trace("window: %zu bytes uncached rc=%d", want, (int)e);
            if (e != hipSuccess) {
                win_ = nullptr;
                return hip_fail(e, "window allocation");
            }
            win_bytes_ = want;
            win_peers_.clear();
        }
        if (win_peers_.empty()) {
            int rc = map_peers(win_, win_peers_);
            if (rc != MPI_SUCCESS) return rc;
        }
        out = win_peers_;
        return MPI_SUCCESS;
    }

    int rma_window(std::vector<char*>& out, size_t* bytes_out) override
    {
        // Collective, first passive-target window of the communicator only:
        // uncached like the engine window (peers write payloads into it)
        if (!rwin_) {
            // ranks sharing this GPU, counted from every rank's PCI bus id
            // (not guessed from WORLD_SIZE / device count: a launcher may show
            // each rank only its own GPU), then the minimum size over ranks
            char bus[64] = {0};
            int dev = 0;
            if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetPCIBusId(bus, (int)sizeof(bus) - 1, dev) != hipSuccess) {
                (void)hipGetLastError();
                snprintf(bus, sizeof(bus), "unknown-%d", rank);
            }
            std::vector<char> buses((size_t)size * sizeof(bus));
            int rc = hub_.allgather(bus, sizeof(bus), buses.data());
            if (rc != MPI_SUCCESS) return rc;
            int share = 0;
            for (int r = 0; r < size; ++r)
                share += strncmp(buses.data() + (size_t)r * sizeof(bus), bus, sizeof(bus)) == 0;
            uint64_t mine = rma_bytes_for(share), lo = mine;
            std::vector<uint64_t> all((size_t)size);
            if ((rc = hub_.allgather(&mine, sizeof(mine), all.data())) != MPI_SUCCESS) return rc;
            for (uint64_t v : all) lo = std::min(lo, v);
            const size_t bytes = (size_t)lo;
            trace("rma window: %d rank(s) on this GPU, %zu bytes here, %zu agreed", share, (size_t)mine, bytes);
            hipError_t e = uc_alloc(bytes, &rwin_);
            trace("rma window: %zu bytes rc=%d", bytes, (int)e);
            if (e != hipSuccess) {
                rwin_ = nullptr;
                return hip_fail(e, "rma staging allocation");
            }
            rc = map_peers(rwin_, rwin_peers_);
            if (rc != MPI_SUCCESS) return rc;
            rbytes_ = bytes;
        }
        out = rwin_peers_;
        *bytes_out = rbytes_;
        return MPI_SUCCESS;
    }

private:
    Hub hub_;
    ShmBarrier shm_;
    hipStream_t stream_ = nullptr;
    unsigned* counter_ = nullptr;
    void* win_ = nullptr;
    size_t win_bytes_ = 0;
    std::vector<char*> win_peers_;
    void* rwin_ = nullptr;                // passive-target staging (rma_window)
    size_t rbytes_ = 0;                   // its agreed size
    std::vector<char*> rwin_peers_;
};

}  // namespace

// Listening socket on an ephemeral loopback port (a derived communicator's hub).
static int listen_ephemeral(int* port)
{
    int fd = socket(AF_INET, SOCK_STREAM, 0);
    if (fd < 0) return -1;
    struct sockaddr_in sa = {};
    sa.sin_family = AF_INET;
    sa.sin_addr.s_addr = htonl(INADDR_LOOPBACK);
    sa.sin_port = 0;
    socklen_t len = sizeof(sa);
    if (bind(fd, (struct sockaddr*)&sa, sizeof(sa)) != 0 || listen(fd, 64) != 0 ||
        getsockname(fd, (struct sockaddr*)&sa, &len) != 0) {
        close(fd);
        return -1;
    }
    *port = ntohs(sa.sin_port);
    return fd;
}

int transport_split(Transport* parent, int color, int key, int* new_rank, int* new_size, Transport** out,
                    std::vector<int>* members_out)
{
    *out = nullptr;
    *new_rank = -1;
    *new_size = 0;
    const int p = parent->size;
    // MPIR_Comm_split: (color, key) of every rank; members of a color ordered
    // by (key, parent rank)
    int32_t mine[2] = {color, key};
    std::vector<int32_t> all((size_t)p * 2);
    int rc = parent->allgather(mine, sizeof(mine), all.data());
    if (rc != MPI_SUCCESS) return rc;
    std::vector<std::pair<std::pair<int, int>, int>> members;   // ((key, parent rank), parent rank)
    if (color != MPI_UNDEFINED)
        for (int r = 0; r < p; ++r)
            if (all[(size_t)r * 2] == color) members.push_back({{all[(size_t)r * 2 + 1], r}, r});
    std::sort(members.begin(), members.end());
    for (size_t i = 0; i < members.size(); ++i)
        if (members[i].second == parent->rank) *new_rank = (int)i;
    *new_size = (int)members.size();
    if (members_out) {
        members_out->clear();
        for (auto& m : members) members_out->push_back(m.second);
    }
    // the new rank 0 of every group of >= 2 opens the group's hub
    int32_t port = 0;
    int lfd = -1;
    if (*new_rank == 0 && *new_size > 1) {
        int pt = 0;
        lfd = listen_ephemeral(&pt);
        port = lfd >= 0 ? pt : -1;
    }
    std::vector<int32_t> ports((size_t)p);
    rc = parent->allgather(&port, sizeof(port), ports.data());
    if (rc != MPI_SUCCESS || *new_size <= 1) {
        if (lfd >= 0) close(lfd);
        return rc;
    }
    const int leader_port = ports[(size_t)members[0].second];
    if (leader_port <= 0) {
        if (lfd >= 0) close(lfd);
        set_error("communicator split: the group's bootstrap socket could not be opened");
        return MPI_ERR_OTHER;
    }
    auto* t = new IpcTransport();
    rc = t->init(*new_rank, *new_size, leader_port, lfd);
    if (rc != MPI_SUCCESS) {
        delete t;
        return rc;
    }
    *out = t;
    return MPI_SUCCESS;
}

int transport_create(int rank, int size, Transport** out)
{
    auto* t = new IpcTransport();
    int rc = t->init(rank, size);
    if (rc != MPI_SUCCESS) {
        delete t;
        return rc;
    }
    *out = t;
    return MPI_SUCCESS;
}

void transport_destroy(Transport* t)
{
    if (!t) return;
    rccl_forget(t);
    if (t->aux) (void)hipStreamDestroy(t->aux);
    delete t;
}

// ===========================================================================
// MPI_Intercomm_create: the union communicator gets an IpcTransport of its
// own, so this one intercommunicator entry point stays beside the class
// (the rest is msx_intercomm.cpp)
// ===========================================================================
int engine_intercomm_create(Comm* local, int leader, Comm* peer, int remote_leader, int tag, Comm** out)
{
    *out = nullptr;
    return worker().run([=]() -> int {
        // 1. rank 0 of each group opens a bootstrap socket; its group learns the port
        int lfd = -1;
        std::vector<int32_t> pv{0};
        if (local->rank == 0) {
            int pt = 0;
            lfd = listen_ephemeral(&pt);
            pv[0] = lfd >= 0 ? pt : -1;
        }
        int rc = group_bcast(local, pv, 0);
        const int32_t gport = pv[0];
        // 2. the leaders swap {leader process id, group port, group size, members}
        std::vector<int32_t> hdr{MPI_SUCCESS, 0, 0, 0}, rem;
        if (rc == MPI_SUCCESS && local->rank == leader) {
            std::vector<int32_t> msg{local->lpid[(size_t)leader], gport, local->size};
            msg.insert(msg.end(), local->lpid.begin(), local->lpid.end());
            const int rl = peer->lpid[(size_t)remote_leader];
            int r2 = mail_send(rl, tag, msg.data(), msg.size() * sizeof(int32_t));
            std::vector<char> got;
            if (r2 == MPI_SUCCESS) r2 = mail_recv(rl, tag, &got);
            if (r2 == MPI_SUCCESS && got.size() >= 3 * sizeof(int32_t)) {
                std::vector<int32_t> g(got.size() / sizeof(int32_t));
                memcpy(g.data(), got.data(), g.size() * sizeof(int32_t));
                hdr = {MPI_SUCCESS, g[0], g[1], g[2]};
                rem.assign(g.begin() + 3, g.end());
            } else {
                hdr[0] = r2 != MPI_SUCCESS ? r2 : MPI_ERR_INTERN;
            }
        }
        if (rc == MPI_SUCCESS) rc = group_bcast(local, hdr, leader);
        if (rc == MPI_SUCCESS && hdr[0] != MPI_SUCCESS) rc = hdr[0];
        if (rc == MPI_SUCCESS && (hdr[2] <= 0 || hdr[3] <= 0)) {
            set_error("MPI_Intercomm_create: the remote group did not publish its bootstrap socket");
            rc = MPI_ERR_OTHER;
        }
        if (rc == MPI_SUCCESS) {
            rem.resize((size_t)hdr[3]);
            rc = group_bcast(local, rem, leader);
        }
        if (rc != MPI_SUCCESS) {
            if (lfd >= 0) close(lfd);
            return rc;
        }
        // 3. both groups in one communicator, the group with the lower leader id first
        const bool low = local->lpid[(size_t)leader] < hdr[1];
        const int nr = hdr[3], nlow = low ? local->size : nr;
        const int usize = local->size + nr, urank = low ? local->rank : nlow + local->rank;
        if (!(low && local->rank == 0) && lfd >= 0) {
            close(lfd);
            lfd = -1;
        }
        auto* t = new IpcTransport();
        rc = t->init(urank, usize, low ? gport : hdr[2], lfd);
        if (rc != MPI_SUCCESS) {
            delete t;
            return rc;
        }
        auto* u = new Comm();
        u->rank = urank;
        u->size = usize;
        u->tp = t;
        u->lpid = low ? local->lpid : rem;
        const std::vector<int>& second = low ? rem : local->lpid;
        u->lpid.insert(u->lpid.end(), second.begin(), second.end());
        rc = map_union(u);
        if (rc != MPI_SUCCESS) {
            free_intra(u);
            return rc;
        }
        // 4. the intercommunicator's own local group
        Comm* lc = nullptr;
        rc = dup_intra(local, &lc);
        if (rc != MPI_SUCCESS) {
            free_intra(u);
            return rc;
        }
        auto* ic = new Comm();
        ic->inter = true;
        ic->rank = local->rank;
        ic->size = local->size;
        ic->lpid = local->lpid;
        ic->remote_lpid.assign(rem.begin(), rem.end());
        ic->is_low = low;
        ic->local = lc;
        ic->uni = u;
        ic->errhandler = local->errhandler;
        *out = ic;
        return MPI_SUCCESS;
    });
}

}  // namespace msx
