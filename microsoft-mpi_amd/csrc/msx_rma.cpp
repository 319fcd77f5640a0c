// msx_rma.cpp — one-sided operations: the fence's target-side apply, the
// passive-target service (lock / unlock / flush) and post-start-complete-wait.
#include "msx_engine.h"

#include <algorithm>
#include <atomic>
#include <fcntl.h>
#include <linux/futex.h>
#include <map>
#include <mutex>
#include <stdio.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/syscall.h>
#include <thread>
#include <unistd.h>

namespace msx {

// ===========================================================================
// one-sided accumulate: target-side application at the fence
// ===========================================================================
namespace {

// target = target (op) origin for `d.count` elements at taddr; the reference's
// do_accumulate_op / MPIDI_Win_local_accumulate (packethandling.cpp:2917-2960,
// win.cpp:1405-1450).  An (op, type) pair outside the op's table reaches
// MPIR_Op_<op>, which only sets op_errno (op.cpp:1791) and leaves the target
// unchanged; nothing reports it, so neither do we.
int rma_combine(const RmaDesc& d, const char* payload, char* taddr, hipStream_t s)
{
    if (d.opidx == O_NOOP || d.count == 0) return MPI_SUCCESS;
    // refused at the origin (rma_op, msx_api_rma.cpp): an accumulate has no fused tree
    if (d.opidx == O_SUM_WIDE) { set_error("MSX_SUM_WIDE is not defined for one-sided calls"); return MPI_ERR_OP; }
    const size_t bytes = (size_t)d.count * (size_t)d.usize;
    if (d.opidx == O_REPLACE) return copy_async(taddr, payload, bytes, s);
    if (op_check_dtype(d.opidx, d.dt) != MPI_SUCCESS) return MPI_SUCCESS;
    const Kind k = type_info(d.dt)->kind;
    if (classify(taddr).place == Place::Device && classify(payload).place == Place::Device) {
        // the streaming combine in place on the target (payloads written by
        // peers sit in uncached window memory, so plain loads see them)
        const hipError_t e = launch_combine(d.opidx, k, payload, taddr, (size_t)d.count, s, LaunchCfg());
        return e == hipSuccess ? MPI_SUCCESS : hip_fail(e, "rma combine");
    }
    int rc = sync_stream(s, "rma");
    return rc == MPI_SUCCESS ? reduce_local_any(d.opidx, k, payload, taddr, (size_t)d.count) : rc;
}

// compare-and-swap of one element (bitwise compare, win.cpp:1909-1990)
int rma_cas(const RmaDesc& d, const char* origin, const char* cmp, char* taddr, char* fetch, hipStream_t s)
{
    const size_t esz = (size_t)d.usize;
    int rc = sync_stream(s, "rma cas");
    char old[16], c[16];
    if (rc == MPI_SUCCESS) rc = copy_any(old, taddr, esz);
    if (rc == MPI_SUCCESS) rc = copy_any(c, cmp, esz);
    if (rc == MPI_SUCCESS && fetch) rc = copy_any(fetch, old, esz);
    if (rc == MPI_SUCCESS && memcmp(old, c, esz) == 0) rc = copy_any(taddr, origin, esz);
    return rc;
}

// A derived target datatype: the gfx950 pack / unpack / accumulate kernels
// walk its layout at taddr (the reference's segment walk of
// packethandling.cpp:2969-3004).  Window memory the GPU cannot address
// (pageable host memory) is staged through HBM around the kernel.
int rma_apply_typed(const RmaDesc& d, const Dtype* T, const char* payload, char* taddr, char* fetch,
                    hipStream_t s)
{
    int64_t lo, hi;
    dt_span(T, d.count, &lo, &hi);
    const BufInfo bi = classify(taddr + lo);
    char* tdev = taddr;
    void* stage = nullptr;
    int rc = MPI_SUCCESS;
    if (bi.place == Place::Device) {
        tdev = static_cast<char*>(bi.dev) - lo;
    } else {
        const size_t span = (size_t)(hi - lo);
        const uintptr_t mis = (uintptr_t)(taddr + lo) & 15;
        if (hipMalloc(&stage, span + 16) != hipSuccess) { set_error("rma staging allocation"); return MPI_ERR_NO_MEM; }
        tdev = static_cast<char*>(stage) + mis - lo;
        rc = copy_async(tdev + lo, taddr + lo, span, s);
    }
    // payload / fetch live in engine windows or device temporaries (device memory)
    if (rc == MPI_SUCCESS && (d.kind == RMA_GET || d.kind == RMA_GACC))
        rc = dt_pack_dev(T, d.count, tdev, fetch, s);
    if (rc == MPI_SUCCESS && (d.kind == RMA_PUT || ((d.kind == RMA_ACC || d.kind == RMA_GACC))))
        rc = d.kind == RMA_PUT ? dt_unpack_dev(T, d.count, payload, tdev, s)
                               : dt_acc_dev(d.opidx, T, d.count, payload, tdev, s);
    if (stage) {
        if (rc == MPI_SUCCESS && d.kind != RMA_GET) rc = copy_async(taddr + lo, tdev + lo, (size_t)(hi - lo), s);
        const int rs = sync_stream(s, "rma typed stage");
        (void)hipFree(stage);
        if (rc == MPI_SUCCESS) rc = rs;
    }
    return rc;
}

// One operation on window memory `taddr` of this rank.  `fetch` receives the
// target's previous contents (GET / GACC / CAS).  T: derived target type or null.
int rma_apply(const RmaDesc& d, const Dtype* T, const char* payload, const char* cmp, char* taddr, char* fetch,
              hipStream_t s)
{
    if (T) return rma_apply_typed(d, T, payload, taddr, fetch, s);
    const size_t bytes = (size_t)d.count * (size_t)d.usize;
    switch (d.kind) {
    case RMA_PUT: return copy_async(taddr, payload, bytes, s);
    case RMA_GET: return copy_async(fetch, taddr, bytes, s);
    case RMA_ACC: return rma_combine(d, payload, taddr, s);
    case RMA_GACC: {
        int rc = copy_async(fetch, taddr, bytes, s);
        return rc == MPI_SUCCESS ? rma_combine(d, payload, taddr, s) : rc;
    }
    case RMA_CAS: return rma_cas(d, payload, cmp, taddr, fetch, s);
    default: set_error("rma: bad operation kind %d", d.kind); return MPI_ERR_INTERN;
    }
}

bool rma_in_bounds(const RmaDesc& d, int64_t winsize)
{
    if (d.tdisp < 0 || d.count < 0 || d.usize <= 0) return false;
    if (d.layout >= 0) return d.tdisp + d.span_lo >= 0 && d.span_hi <= winsize - d.tdisp;
    const int64_t n = (d.kind == RMA_CAS) ? 1 : d.count;
    if (n > (INT64_MAX - d.tdisp) / d.usize) return false;
    return d.tdisp + n * d.usize <= winsize;
}

hipStream_t rma_self_stream()
{
    static hipStream_t s = [] {
        hipStream_t t = nullptr;
        (void)hipStreamCreateWithFlags(&t, hipStreamNonBlocking);
        return t;
    }();
    return s;
}

// A slice [lo, hi) of one queued operation, staged through the engine
// windows: payload in the target's IN area, fetched bytes in the origin's OUT.
struct RmaPiece {
    int origin;
    int64_t idx;           // index in the origin's queue
    int64_t lo, hi;        // unit range
    size_t in_off, out_off;
    size_t in_b, out_b;
};

struct TypeCache {         // standalone target layouts rebuilt at this rank
    std::map<std::pair<int, int64_t>, Dtype*> m;
    ~TypeCache()
    {
        for (auto& kv : m) dtype_delete(kv.second);
    }
};

int do_rma_fence(RmaWin* win)
{
    Comm* c = win->comm;
    Transport* tp = c->tp;
    const int p = c->size, me = c->rank;
    int rc = ensure_device();
    if (rc != MPI_SUCCESS) return rc;
    // 1. every origin's queue and derived-layout blob, on every rank
    int64_t mine[2] = {(int64_t)win->q.size(), (int64_t)win->blob.size()};
    std::vector<int64_t> ns((size_t)p * 2);
    if ((rc = tp->allgather(mine, sizeof(mine), ns.data())) != MPI_SUCCESS) return rc;
    int64_t maxn = 0, maxb = 0;
    for (int r = 0; r < p; ++r) {
        maxn = std::max(maxn, ns[(size_t)r * 2]);
        maxb = std::max(maxb, ns[(size_t)r * 2 + 1]);
    }
    trace("rma fence: %lld local ops, max %lld", (long long)mine[0], (long long)maxn);
    if (maxn == 0) return tp->barrier();
    std::vector<RmaDesc> padded((size_t)maxn), all((size_t)p * (size_t)maxn);
    std::copy(win->q.begin(), win->q.end(), padded.begin());
    if ((rc = tp->allgather(padded.data(), (size_t)maxn * sizeof(RmaDesc), all.data())) != MPI_SUCCESS) return rc;
    std::vector<int64_t> blobs;
    if (maxb > 0) {
        std::vector<int64_t> pb((size_t)maxb, 0);
        std::copy(win->blob.begin(), win->blob.end(), pb.begin());
        blobs.resize((size_t)p * (size_t)maxb);
        if ((rc = tp->allgather(pb.data(), (size_t)maxb * sizeof(int64_t), blobs.data())) != MPI_SUCCESS) return rc;
    }
    TypeCache types;
    auto target_type = [&](int o, int64_t i, const RmaDesc& d) -> const Dtype* {
        if (d.layout < 0) return nullptr;
        auto key = std::make_pair(o, i);
        auto it = types.m.find(key);
        if (it != types.m.end()) return it->second;
        Dtype* t = dtype_from_blob(blobs.data() + (size_t)o * maxb + d.layout, ns[(size_t)o * 2 + 1] - d.layout);
        types.m[key] = t;
        return t;
    };
    Windows w;
    if ((rc = get_windows(tp, &w)) != MPI_SUCCESS) return rc;
    const size_t C = w.C;
    // 2. cut operations into pieces and pack them into rounds; a target
    //    applies its pieces in (origin, issue) order, round after round
    std::vector<std::vector<RmaPiece>> rounds(1);
    std::vector<size_t> in_used((size_t)p, 0), out_used((size_t)p, 0);
    int my_err = MPI_SUCCESS;
    for (int o = 0; o < p; ++o) {
        for (int64_t i = 0; i < ns[(size_t)o * 2]; ++i) {
            const RmaDesc& d = all[(size_t)o * maxn + i];
            const size_t esz = (size_t)d.usize;
            if (!rma_in_bounds(d, win->sizes[(size_t)d.target])) {
                // packethandling.cpp:1339-1383: **requestrmaoutofbounds
                if (o == me) {
                    my_err = MPI_ERR_REQUEST;
                    set_error("RMA operation outside the target window (target %d, disp %lld)", d.target,
                              (long long)d.tdisp);
                }
                continue;
            }
            if (esz > C / 2) {
                if (o == me) {
                    my_err = MPI_ERR_TYPE;
                    set_error("RMA target datatype of %zu bytes exceeds the staging window", esz);
                }
                continue;
            }
            const int64_t n = (d.kind == RMA_CAS) ? 1 : d.count;
            const bool sends = d.kind == RMA_PUT || d.kind == RMA_CAS || ((d.kind == RMA_ACC || d.kind == RMA_GACC) && d.opidx != O_NOOP);
            const bool fetches = d.kind == RMA_GET || d.kind == RMA_GACC || d.kind == RMA_CAS;
            int64_t per = (int64_t)(C / esz / 2) & ~(int64_t)15;
            if (per <= 0) per = 1;
            for (int64_t lo = 0; lo < n; lo += per) {
                const int64_t hi = std::min(n, lo + per);
                RmaPiece pc;
                pc.origin = o;
                pc.idx = i;
                pc.lo = lo;
                pc.hi = hi;
                pc.in_b = sends ? (size_t)(hi - lo) * esz * (d.kind == RMA_CAS ? 2 : 1) : 0;
                pc.out_b = fetches ? (size_t)(hi - lo) * esz : 0;
                const size_t ia = (pc.in_b + 255) & ~(size_t)255, oa = (pc.out_b + 255) & ~(size_t)255;
                if (in_used[(size_t)d.target] + ia > C || out_used[(size_t)o] + oa > C) {
                    rounds.emplace_back();
                    std::fill(in_used.begin(), in_used.end(), 0);
                    std::fill(out_used.begin(), out_used.end(), 0);
                }
                pc.in_off = in_used[(size_t)d.target];
                pc.out_off = out_used[(size_t)o];
                in_used[(size_t)d.target] += ia;
                out_used[(size_t)o] += oa;
                rounds.back().push_back(pc);
            }
        }
    }
    hipStream_t s = tp->stream();
    for (const auto& round : rounds) {
        // a. origins write payloads into the targets' IN areas (xGMI writes)
        for (const RmaPiece& pc : round) {
            if (pc.origin != me || !pc.in_b) continue;
            const RmaDesc& d = all[(size_t)me * maxn + pc.idx];
            const RmaLocal& l = win->ql[(size_t)pc.idx];
            const size_t esz = (size_t)d.usize;
            char* dst = w.in(d.target) + pc.in_off;
            if (d.kind == RMA_CAS) {
                rc = copy_async(dst, l.origin, esz, s);
                if (rc == MPI_SUCCESS) rc = copy_async(dst + esz, l.compare, esz, s);
            } else {
                rc = copy_async(dst, static_cast<const char*>(l.origin) + pc.lo * esz, pc.in_b, s);
            }
            if (rc != MPI_SUCCESS) return rc;
        }
        if ((rc = sync_stream(s, "rma payload")) != MPI_SUCCESS) return rc;
        if ((rc = tp->barrier()) != MPI_SUCCESS) return rc;
        // b. targets apply in (origin, issue) order; fetched bytes go to the
        //    origin's OUT area
        for (const RmaPiece& pc : round) {
            const RmaDesc& d0 = all[(size_t)pc.origin * maxn + pc.idx];
            if (d0.target != me) continue;
            const Dtype* T = target_type(pc.origin, pc.idx, d0);
            if (d0.layout >= 0 && !T) { set_error("rma: malformed datatype layout"); return MPI_ERR_INTERN; }
            RmaDesc d = d0;
            d.count = (d0.kind == RMA_CAS) ? 1 : pc.hi - pc.lo;
            char* taddr = win->base + d0.tdisp + pc.lo * d0.uext;
            const char* payload = w.in(me) + pc.in_off;
            char* fetch = pc.out_b ? w.out(pc.origin) + pc.out_off : nullptr;
            rc = rma_apply(d, T, payload, payload + d0.usize, taddr, fetch, s);
            if (rc != MPI_SUCCESS) return rc;
        }
        if ((rc = sync_stream(s, "rma apply")) != MPI_SUCCESS) return rc;
        if ((rc = tp->barrier()) != MPI_SUCCESS) return rc;
        // c. origins deliver fetched values to their result buffers
        for (const RmaPiece& pc : round) {
            if (pc.origin != me || !pc.out_b) continue;
            const RmaDesc& d = all[(size_t)me * maxn + pc.idx];
            rc = copy_async(static_cast<char*>(win->ql[(size_t)pc.idx].result) + pc.lo * d.usize,
                            w.out(me) + pc.out_off, pc.out_b, s);
            if (rc != MPI_SUCCESS) return rc;
        }
        if ((rc = sync_stream(s, "rma deliver")) != MPI_SUCCESS) return rc;
    }
    for (RmaLocal& l : win->ql) {
        const int r2 = rma_local_complete(l);
        if (rc == MPI_SUCCESS) rc = r2;
    }
    win->q.clear();
    win->ql.clear();
    win->blob.clear();
    trace("rma fence: %zu rounds done", rounds.size());
    return rc != MPI_SUCCESS ? rc : my_err;
}

}  // namespace

int rma_local_complete(RmaLocal& l)
{
    int rc = MPI_SUCCESS;
    if (l.tmp_result) {
        // a derived result type: the fetched bytes arrived packed
        Dtype* t = dtype_lookup(l.result_dt);
        rc = t ? dt_unpack_any(t, l.result_count, l.tmp_result, l.result_user) : MPI_ERR_TYPE;
        (void)hipFree(l.tmp_result);
        l.tmp_result = nullptr;
        MPI_Datatype h = l.result_dt;
        if (dtype_is_derived(h)) dtype_free(&h);     // the reference taken at issue
    }
    if (l.tmp_origin) {
        (void)hipFree(l.tmp_origin);
        l.tmp_origin = nullptr;
    }
    return rc;
}

int rma_apply_self(RmaWin* w, const RmaDesc& d, const RmaLocal& l, const Dtype* T)
{
    int rc = ensure_device();
    if (rc != MPI_SUCCESS) return rc;
    if (!rma_in_bounds(d, w->size)) {
        set_error("RMA operation outside the window (disp %lld)", (long long)d.tdisp);
        return MPI_ERR_REQUEST;
    }
    hipStream_t s = rma_self_stream();
    rc = rma_apply(d, T, static_cast<const char*>(l.origin), static_cast<const char*>(l.compare),
                   w->base + d.tdisp, static_cast<char*>(l.result), s);
    return rc == MPI_SUCCESS ? sync_stream(s, "rma self") : rc;
}

namespace {
int passive_init(RmaWin* w);   // below, with the passive-target machinery
}

int engine_rma_create(RmaWin* w)
{
    Comm* c = w->comm;
    const int p = c->size;
    w->sizes.assign((size_t)p, 0);
    w->disp_units.assign((size_t)p, 1);
    if (p == 1 || !c->tp) {
        w->sizes[0] = w->size;
        w->disp_units[0] = w->disp_unit;
        return MPI_SUCCESS;
    }
    return worker().run([w, c, p] {
        int64_t mine[2] = {w->size, (int64_t)w->disp_unit};
        std::vector<int64_t> all((size_t)p * 2);
        int rc = c->tp->allgather(mine, sizeof(mine), all.data());
        for (int r = 0; rc == MPI_SUCCESS && r < p; ++r) {
            w->sizes[(size_t)r] = all[(size_t)r * 2];
            w->disp_units[(size_t)r] = (int)all[(size_t)r * 2 + 1];
        }
        // passive target: mailbox + this rank's service thread (collective)
        if (rc == MPI_SUCCESS) rc = passive_init(w);
        return rc;
    });
}

// ---- passive target (MPI_Win_lock / unlock / flush) -----------------------------
struct PassiveReq {               // one request of a mailbox slot (plain data)
    RmaDesc d;                    // this piece: count, tdisp of its first unit
    int64_t blob_n = 0;           // int64 words of target layout at the payload slot's start
    int64_t payload_off = 0;      // payload bytes in the slot (after the layout)
    int32_t has_fetch = 0;
    int32_t pad_ = 0;
};
struct PassiveSlot {              // mailbox slot (target t, origin o)
    std::atomic<uint32_t> req;    // origin: +1 after writing r
    std::atomic<uint32_t> done;   // target: = req once applied
    std::atomic<int32_t> rc;
    int32_t pad_;
    PassiveReq r;
};

struct PassiveState {
    RmaWin* w = nullptr;
    int p = 1, me = 0;
    Windows win;                          // the communicator's engine windows
    void* shm = nullptr;
    size_t shm_bytes = 0;
    std::atomic<uint32_t>* door = nullptr;    // per target: doorbell of its service thread
    std::atomic<int32_t>* lock = nullptr;     // per target: 0 free, > 0 readers, -1 writer
    PassiveSlot* slots = nullptr;             // [target * p + origin]
    std::atomic<uint32_t>* post = nullptr;    // [target * p + origin]: exposure epochs posted
    std::atomic<uint32_t>* cmpl = nullptr;    // [target * p + origin]: access epochs completed
    std::thread th;
    std::atomic<bool> stop{false};
    std::mutex apply_mu;                      // service thread vs. self-target applies
    hipStream_t os = nullptr;                 // origin-side copies
};

void futex_wake_all(void* addr)
{
    syscall(SYS_futex, reinterpret_cast<uint32_t*>(addr), FUTEX_WAKE, INT32_MAX, nullptr, nullptr, 0);
}

void futex_wait_ms(void* addr, uint32_t val, long ms)
{
    struct timespec ts = {ms / 1000, (ms % 1000) * 1000000};
    syscall(SYS_futex, reinterpret_cast<uint32_t*>(addr), FUTEX_WAIT, val, &ts, nullptr, 0);
}

// A shared-memory segment of `bytes` mapped by every rank (collective).
int shm_collective(Transport* tp, size_t bytes, void** out)
{
    *out = nullptr;
    static std::atomic<int> serial{0};
    char name[64] = {0};
    if (tp->rank == 0)
        snprintf(name, sizeof(name), "/msx_win_%d_%d_%ld", (int)getpid(), serial.fetch_add(1),
                 (long)(now_s() * 1e6) % 1000000000L);
    // rank 0 creates and sizes the segment BEFORE anyone learns its name
    int fd = -1;
    if (tp->rank == 0) {
        fd = shm_open(name, O_CREAT | O_RDWR, 0600);
        if (fd < 0 || ftruncate(fd, (off_t)bytes) != 0) name[0] = 0;
    }
    std::vector<char> all((size_t)tp->size * sizeof(name));
    int rc = tp->allgather(name, sizeof(name), all.data());
    if (rc != MPI_SUCCESS) {
        if (fd >= 0) close(fd);
        return rc;
    }
    memcpy(name, all.data(), sizeof(name));
    int ok = name[0] != 0;
    if (ok && tp->rank != 0) fd = shm_open(name, O_RDWR, 0600);
    std::vector<int> oks((size_t)tp->size);
    void* m = MAP_FAILED;
    if (ok && fd >= 0) m = mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
    if (fd >= 0) close(fd);
    int mine = m != MAP_FAILED ? 1 : 0;
    rc = tp->allgather(&mine, sizeof(int), oks.data());
    if (tp->rank == 0) shm_unlink(name);
    bool all_ok = rc == MPI_SUCCESS && mine;
    for (int v : oks) all_ok = all_ok && v;
    if (!all_ok) {
        if (m != MAP_FAILED) munmap(m, bytes);
        set_error("passive target: shared-memory mailbox unavailable");
        return rc != MPI_SUCCESS ? rc : MPI_ERR_NO_MEM;
    }
    *out = m;                     // zero-filled by ftruncate
    return MPI_SUCCESS;
}

namespace {

// Target side: apply one request of origin o to this rank's window memory.
int passive_apply(PassiveState* ps, int o, const PassiveReq& r, hipStream_t s)
{
    std::lock_guard<std::mutex> g(ps->apply_mu);
    const RmaDesc& d = r.d;
    const char* slot = ps->win.rma_in(ps->me, o);
    Dtype* T = nullptr;
    if (r.blob_n > 0) {
        std::vector<int64_t> blob((size_t)r.blob_n);
        int rc = copy_any(blob.data(), slot, (size_t)r.blob_n * sizeof(int64_t));
        if (rc != MPI_SUCCESS) return rc;
        T = dtype_from_blob(blob.data(), r.blob_n);
        if (!T) { set_error("passive target: malformed datatype layout"); return MPI_ERR_INTERN; }
    }
    const char* payload = slot + r.payload_off;
    char* fetch = r.has_fetch ? ps->win.rma_fetch(o, ps->me) : nullptr;
    int rc = rma_apply(d, T, payload, payload + d.usize, ps->w->base + d.tdisp, fetch, s);
    const int rs = sync_stream(s, "passive apply");
    if (T) dtype_delete(T);
    return rc != MPI_SUCCESS ? rc : rs;
}

// The service thread of one window: applies every origin's requests in
// arrival order, whatever this rank's own thread is doing.
void passive_serve(PassiveState* ps)
{
    (void)ensure_device();
    hipStream_t s = nullptr;
    (void)hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    std::atomic<uint32_t>& door = ps->door[ps->me];
    for (;;) {
        const uint32_t d0 = door.load(std::memory_order_acquire);
        bool any = false;
        for (int o = 0; o < ps->p; ++o) {
            PassiveSlot& sl = ps->slots[(size_t)ps->me * ps->p + o];
            const uint32_t q = sl.req.load(std::memory_order_acquire);
            if (q == sl.done.load(std::memory_order_relaxed)) continue;
            any = true;
            const int rc = s ? passive_apply(ps, o, sl.r, s) : MPI_ERR_OTHER;
            sl.rc.store(rc, std::memory_order_relaxed);
            sl.done.store(q, std::memory_order_release);
            futex_wake_all(&sl.done);
        }
        if (any) continue;
        if (ps->stop.load(std::memory_order_acquire)) break;
        futex_wait_ms(&door, d0, 100);
    }
    if (s) (void)hipStreamDestroy(s);
}

int passive_lock(PassiveState* ps, int t, int mode)
{
    std::atomic<int32_t>& lk = ps->lock[t];
    const double t_end = now_s() + 600.0;
    for (int spin = 0;; ++spin) {
        int32_t v = lk.load(std::memory_order_acquire);
        if (mode == MPI_LOCK_EXCLUSIVE ? v == 0 : v >= 0) {
            const int32_t nv = mode == MPI_LOCK_EXCLUSIVE ? -1 : v + 1;
            if (lk.compare_exchange_weak(v, nv, std::memory_order_acq_rel)) return MPI_SUCCESS;
            continue;
        }
        if (now_s() > t_end) {
            set_error("MPI_Win_lock: lock of rank %d not granted within 600 s", t);
            return MPI_ERR_OTHER;
        }
        if (spin < 1000) sched_yield();
        else futex_wait_ms(&lk, (uint32_t)v, 10);
    }
}

void passive_unlock(PassiveState* ps, int t, int mode)
{
    std::atomic<int32_t>& lk = ps->lock[t];
    if (mode == MPI_LOCK_EXCLUSIVE) lk.store(0, std::memory_order_release);
    else lk.fetch_sub(1, std::memory_order_acq_rel);
    futex_wake_all(&lk);
}

// Origin side: ship one queued operation to target t piece by piece (payload
// slot capacity) and wait for each piece to be applied.
int passive_ship(PassiveState* ps, int t, const RmaDesc& d0, const RmaLocal& l, const int64_t* blob, int64_t blob_n)
{
    const size_t S = ps->win.rma_slot();
    const size_t blob_b = ((size_t)blob_n * sizeof(int64_t) + 255) & ~(size_t)255;
    const bool sends = d0.kind == RMA_PUT || d0.kind == RMA_CAS ||
                       ((d0.kind == RMA_ACC || d0.kind == RMA_GACC) && d0.opidx != O_NOOP);
    const bool fetches = d0.kind == RMA_GET || d0.kind == RMA_GACC || d0.kind == RMA_CAS;
    const size_t esz = (size_t)d0.usize;
    const size_t unit_in = sends ? esz * (d0.kind == RMA_CAS ? 2 : 1) : 0;
    if (blob_b + unit_in > S || esz > S) {
        set_error("passive target: a %zu-byte unit does not fit the %zu-byte staging slot", esz, S);
        return MPI_ERR_TYPE;
    }
    const int64_t n = d0.kind == RMA_CAS ? 1 : d0.count;
    int64_t per = unit_in ? (int64_t)((S - blob_b) / unit_in) : n;
    if (fetches) per = std::min<int64_t>(per, (int64_t)(S / esz));
    per = std::max<int64_t>(per, 1);
    char* dst = ps->win.rma_in(t, ps->me);
    PassiveSlot& sl = ps->slots[(size_t)t * ps->p + ps->me];
    int rc = MPI_SUCCESS;
    for (int64_t lo = 0; lo < n && rc == MPI_SUCCESS; lo += per) {
        const int64_t hi = std::min(n, lo + per);
        if (blob_n) rc = copy_async(dst, blob, (size_t)blob_n * sizeof(int64_t), ps->os);
        if (rc == MPI_SUCCESS && sends) {
            if (d0.kind == RMA_CAS) {
                rc = copy_async(dst + blob_b, l.origin, esz, ps->os);
                if (rc == MPI_SUCCESS) rc = copy_async(dst + blob_b + esz, l.compare, esz, ps->os);
            } else {
                rc = copy_async(dst + blob_b, static_cast<const char*>(l.origin) + lo * esz, (size_t)(hi - lo) * esz,
                                ps->os);
            }
        }
        if (rc == MPI_SUCCESS) rc = sync_stream(ps->os, "passive payload");
        if (rc != MPI_SUCCESS) break;
        PassiveReq& r = sl.r;
        r.d = d0;
        r.d.count = d0.kind == RMA_CAS ? 1 : hi - lo;
        r.d.tdisp = d0.tdisp + lo * d0.uext;
        r.d.layout = blob_n ? 0 : -1;
        r.blob_n = blob_n;
        r.payload_off = (int64_t)blob_b;
        r.has_fetch = fetches ? 1 : 0;
        const uint32_t q = sl.req.load(std::memory_order_relaxed) + 1;
        sl.req.store(q, std::memory_order_release);
        ps->door[t].fetch_add(1, std::memory_order_acq_rel);
        futex_wake_all(&ps->door[t]);
        const double t_end = now_s() + 600.0;
        for (int spin = 0;; ++spin) {
            const uint32_t dn = sl.done.load(std::memory_order_acquire);
            if (dn == q) break;
            if (now_s() > t_end) {
                set_error("passive target: rank %d did not apply within 600 s", t);
                return MPI_ERR_OTHER;
            }
            if (spin < 2000) sched_yield();
            else futex_wait_ms(&sl.done, dn, 10);
        }
        rc = sl.rc.load(std::memory_order_relaxed);
        if (rc == MPI_SUCCESS && fetches)
            rc = copy_async(static_cast<char*>(l.result) + lo * esz, ps->win.rma_fetch(ps->me, t),
                            (size_t)(hi - lo) * esz, ps->os);
        if (rc == MPI_SUCCESS && fetches) rc = sync_stream(ps->os, "passive fetch");
    }
    return rc;
}

int passive_init(RmaWin* w)
{
    Comm* c = w->comm;
    auto* ps = new PassiveState();
    ps->w = w;
    ps->p = c->size;
    ps->me = c->rank;
    int rc = get_windows(c->tp, &ps->win);
    if (rc == MPI_SUCCESS) rc = c->tp->rma_window(ps->win.rbase, &ps->win.rbytes);
    const size_t p = (size_t)ps->p;
    const size_t hdr = ((p * sizeof(std::atomic<uint32_t>) + p * sizeof(std::atomic<int32_t>)) + 63) & ~(size_t)63;
    const size_t pscw = (2 * p * p * sizeof(std::atomic<uint32_t>) + 63) & ~(size_t)63;
    ps->shm_bytes = hdr + p * p * sizeof(PassiveSlot) + pscw;
    if (rc == MPI_SUCCESS) rc = shm_collective(c->tp, ps->shm_bytes, &ps->shm);
    if (rc == MPI_SUCCESS && hipStreamCreateWithFlags(&ps->os, hipStreamNonBlocking) != hipSuccess) {
        set_error("passive target: stream creation failed");
        rc = MPI_ERR_OTHER;
    }
    if (rc != MPI_SUCCESS) {
        if (ps->shm) munmap(ps->shm, ps->shm_bytes);
        delete ps;
        return rc;
    }
    char* base = static_cast<char*>(ps->shm);
    ps->door = reinterpret_cast<std::atomic<uint32_t>*>(base);
    ps->lock = reinterpret_cast<std::atomic<int32_t>*>(base + p * sizeof(std::atomic<uint32_t>));
    ps->slots = reinterpret_cast<PassiveSlot*>(base + hdr);
    ps->post = reinterpret_cast<std::atomic<uint32_t>*>(base + hdr + p * p * sizeof(PassiveSlot));
    ps->cmpl = ps->post + p * p;
    ps->th = std::thread(passive_serve, ps);
    w->passive = ps;
    return MPI_SUCCESS;
}

}  // namespace

int engine_rma_free(RmaWin* w)
{
    PassiveState* ps = w->passive;
    if (!ps) return MPI_SUCCESS;
    ps->stop.store(true, std::memory_order_release);
    ps->door[ps->me].fetch_add(1, std::memory_order_acq_rel);
    futex_wake_all(&ps->door[ps->me]);
    if (ps->th.joinable()) ps->th.join();
    if (ps->os) (void)hipStreamDestroy(ps->os);
    munmap(ps->shm, ps->shm_bytes);
    delete ps;
    w->passive = nullptr;
    return MPI_SUCCESS;
}

int engine_rma_lock(RmaWin* w, int target, int mode)
{
    return w->passive ? passive_lock(w->passive, target, mode) : MPI_SUCCESS;
}

int engine_rma_unlock_target(RmaWin* w, int target)
{
    if (w->passive && w->lock_held[(size_t)target]) passive_unlock(w->passive, target, w->lock_mode[(size_t)target]);
    return MPI_SUCCESS;
}

int engine_rma_flush(RmaWin* w, int target)
{
    PassiveState* ps = w->passive;
    if (!ps) return MPI_SUCCESS;                    // one rank: every operation was applied at its call
    int rc = MPI_SUCCESS;
    bool pending = false;
    for (const RmaDesc& d : w->q) pending = pending || d.target == target;
    if (!pending) return MPI_SUCCESS;
    if (w->lock_mode[(size_t)target] && !w->lock_held[(size_t)target]) {
        // the lazily requested lock is granted now
        if ((rc = passive_lock(ps, target, w->lock_mode[(size_t)target])) != MPI_SUCCESS) return rc;
        w->lock_held[(size_t)target] = 1;
    }
    std::vector<RmaDesc> keep_q;
    std::vector<RmaLocal> keep_l;
    for (size_t i = 0; i < w->q.size(); ++i) {
        const RmaDesc& d = w->q[i];
        if (d.target != target) {
            keep_q.push_back(d);
            keep_l.push_back(w->ql[i]);
            continue;
        }
        int r2 = MPI_SUCCESS;
        if (!rma_in_bounds(d, w->sizes[(size_t)target])) {
            set_error("RMA operation outside the target window (target %d, disp %lld)", target, (long long)d.tdisp);
            r2 = MPI_ERR_REQUEST;                   // packethandling.cpp:1339-1383
        } else if (rc == MPI_SUCCESS) {
            const int64_t* blob = d.layout >= 0 ? w->blob.data() + d.layout : nullptr;
            const int64_t blob_n = d.layout >= 0 ? (int64_t)w->blob.size() - d.layout : 0;
            r2 = passive_ship(ps, target, d, w->ql[i], blob, blob_n);
        }
        const int r3 = rma_local_complete(w->ql[i]);
        if (rc == MPI_SUCCESS) rc = r2 != MPI_SUCCESS ? r2 : r3;
    }
    w->q.swap(keep_q);
    w->ql.swap(keep_l);
    if (w->q.empty()) w->blob.clear();
    return rc;
}

namespace {
// Block until *word >= want (shared memory, another process bumps it).
int wait_counter(std::atomic<uint32_t>* word, uint32_t want, const char* what, int peer)
{
    const double t_end = now_s() + 600.0;
    for (int spin = 0;; ++spin) {
        const uint32_t v = word->load(std::memory_order_acquire);
        if ((int32_t)(v - want) >= 0) return MPI_SUCCESS;
        if (now_s() > t_end) {
            set_error("%s: rank %d did not synchronise within 600 s", what, peer);
            return MPI_ERR_OTHER;
        }
        if (spin < 2000) sched_yield();
        else futex_wait_ms(word, v, 10);
    }
}
}  // namespace

int engine_rma_post(RmaWin* w)
{
    PassiveState* ps = w->passive;
    for (int o : w->exposure_origins) {
        w->posts[(size_t)o] += 1;
        if (!ps) continue;                         // one rank: nothing to tell
        std::atomic<uint32_t>& word = ps->post[(size_t)ps->me * ps->p + o];
        word.fetch_add(1, std::memory_order_acq_rel);
        futex_wake_all(&word);
    }
    return MPI_SUCCESS;
}

int engine_rma_complete(RmaWin* w)
{
    PassiveState* ps = w->passive;
    int rc = MPI_SUCCESS;
    for (int t : w->access_targets) {
        w->starts[(size_t)t] += 1;
        if (!ps) continue;                         // one rank: every operation was applied at its call
        // MPID_Win_complete (win.cpp:3859-3874): the target's post first
        if (t != ps->me && !(w->access_assert & MPI_MODE_NOCHECK)) {
            const int r2 = wait_counter(&ps->post[(size_t)t * ps->p + ps->me], w->starts[(size_t)t],
                                        "MPI_Win_complete", t);
            if (rc == MPI_SUCCESS) rc = r2;
            if (r2 != MPI_SUCCESS) continue;
        }
        const int r3 = engine_rma_flush(w, t);     // applied at the target before it is counted
        if (rc == MPI_SUCCESS) rc = r3;
        std::atomic<uint32_t>& word = ps->cmpl[(size_t)t * ps->p + ps->me];
        word.fetch_add(1, std::memory_order_acq_rel);
        futex_wake_all(&word);
    }
    return rc;
}

int engine_rma_wait(RmaWin* w, bool block, int* flag)
{
    PassiveState* ps = w->passive;
    *flag = 1;
    if (!ps) return MPI_SUCCESS;
    for (int o : w->exposure_origins) {
        std::atomic<uint32_t>* word = &ps->cmpl[(size_t)ps->me * ps->p + o];
        const uint32_t want = w->posts[(size_t)o];
        if (!block) {
            if ((int32_t)(word->load(std::memory_order_acquire) - want) < 0) { *flag = 0; return MPI_SUCCESS; }
            continue;
        }
        const int rc = wait_counter(word, want, "MPI_Win_wait", o);
        if (rc != MPI_SUCCESS) return rc;
    }
    return MPI_SUCCESS;
}

void engine_rma_self_guard(RmaWin* w, bool enter)
{
    if (!w->passive) return;
    if (enter) w->passive->apply_mu.lock();
    else w->passive->apply_mu.unlock();
}

int engine_rma_fence(RmaWin* w)
{
    if (w->comm->size == 1 || !w->comm->tp) return MPI_SUCCESS;   // all operations were local
    return worker().run([w] { return do_rma_fence(w); });
}

}  // namespace msx
