// msx_engine.cpp — what every engine path stands on: the collective worker
// thread, flag-wait diagnostics, the tree launch, the user-op host path,
// window geometry, bounce buffers, copies, and the engine's statistics and
// probes.  Shared declarations: msx_engine.h.
#include "msx_engine.h"

#include <algorithm>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

namespace msx {

// ===========================================================================
// engine
// ===========================================================================
Worker& worker()
{
    static Worker w;
    return w;
}

// A GPU flag wait ran out of time: the kernel stored tag * 65536 + 1 + r
// into the pinned word (r = the first flag index still missing; for the
// collectives' per-rank flags, the peer's rank).  One structured line, the
// text of msx_last_error(), which bench_collectives.py parses into its JSON.
int flag_timeout(const char* op, int me, int word, unsigned long long seq, bool index_is_rank)
{
    const int tag = word >> 16, idx = (word & 0xffff) - 1;
    const char* phase = tag == 2 ? "result" : (tag == 3 ? "half_free" : "arrival");
    set_error("flag timeout: op=%s rank=%d phase=%s peer=%d seq=%llu limit_s=%.1f", op, me, phase,
              index_is_rank ? idx : -1, seq, flag_wait_seconds());
    trace("%s", last_error());
    return MPI_ERR_OTHER;
}

// Fault injection for the timeout diagnostics (test hook):
// MSX_TEST_DROP_FLAGS=<rank>:<seq> -- that rank does not post its arrival
// flags of flag-synchronised call <seq>, so its peers' waits run out.
bool fault_drop_flags(int me, unsigned long long seq)
{
    static const std::pair<int, unsigned long long> f = [] {
        const char* e = getenv("MSX_TEST_DROP_FLAGS");
        int r = -1;
        unsigned long long q = 0;
        if (e && sscanf(e, "%d:%llu", &r, &q) != 2) r = -1;
        return std::make_pair(r, q);
    }();
    if (f.first != me || f.second != seq) return false;
    trace("fault injection: rank %d drops the arrival flags of call %llu", me, seq);
    return true;
}

int sync_stream(hipStream_t s, const char* what)
{
    PhaseScope ph(what, -1, true);
    hipError_t e = hipStreamSynchronize(s);
    return e == hipSuccess ? MPI_SUCCESS : hip_fail(e, what);
}

// Evaluate RankTree `t` over [start, start+len) elements of the per-rank
// source pointers `srcs` into `out`.
int run_rank_tree(int opidx, Kind k, const RankTree& t, const std::vector<char*>& srcs, size_t esz,
                  size_t start, size_t len, char* out, hipStream_t s,
                  const std::vector<char*>& extra_outs, const TreeWait* wait)
{
    if (len == 0) return MPI_SUCCESS;
    TreeSpec spec;
    if (wait) {
        if (wait->done_counter) {
            const size_t nf = wait->done_flags ? wait->done_flags->size() : 0;
            if (nf > 64) { set_error("result flags: too many peers"); return MPI_ERR_INTERN; }
            spec.done_counter = wait->done_counter;
            spec.done_launches = wait->done_launches;
            spec.done_nflags = (int)nf;
            for (size_t i = 0; i < nf; ++i) spec.done_flags[i] = (*wait->done_flags)[i];
            spec.done_seq = wait->done_seq;
        }
    }
    if (extra_outs.size() > 31) { set_error("tree combine: too many destinations"); return MPI_ERR_INTERN; }
    spec.nextra = (int)extra_outs.size();
    for (size_t e = 0; e < extra_outs.size(); ++e) spec.extra[e] = extra_outs[e];
    spec.P = t.P;
    spec.nleaves = t.nleaves;
    spec.pairmask = t.pairmask;
    spec.chain = t.chain;
    const int nslots = t.chain ? t.P : 2 * (t.nleaves ? t.nleaves : t.P);
    for (int i = 0; i < nslots; ++i)
        spec.src[i] = t.src[i] >= 0 ? srcs[(size_t)t.src[i]] + start * esz : nullptr;
    hipError_t e = launch_tree_spec(opidx, k, spec, out, len, s);
    return e == hipSuccess ? MPI_SUCCESS : hip_fail(e, "tree combine");
}

// ---- host path for user-defined ops --------------------------------------
// User functions are host code; every contribution is gathered to host memory
// as an IMAGE: the bytes `count` elements of `dt` span.  For a predefined type
// that is the packed array; for a derived datatype (which only user ops
// accept, the builtin check tables reject it) it is the typed byte span, so
// the user function sees the layout it was written for.  Pointers handed
// around below are TYPED BASES (image start - lo), like the user's buffers.
Img img_of(MPI_Datatype dt, size_t count)
{
    Img m;
    if (dtype_is_derived(dt)) {
        m.t = dtype_lookup(dt);
        int64_t lo, hi;
        dt_span(m.t, (int64_t)count, &lo, &hi);
        m.lo = lo;
        m.bytes = (size_t)(hi - lo);
    } else {
        m.esz = (size_t)type_size(dt);
        m.bytes = count * m.esz;
    }
    return m;
}

// image <- buf (any memory)
int img_load(const Img& m, const void* buf, char* img)
{
    return copy_any(img, static_cast<const char*>(buf) + m.lo, m.bytes);
}

// buf <- image: a derived type writes only the bytes its type map covers
// (MPIR_Localcopy through the type, gaps of `buf` untouched): the mapped bytes
// are gathered on the host and the GPU unpack kernel scatters them.
int img_store(const Img& m, size_t count, const char* typed_base, void* buf)
{
    if (!m.t) return copy_any(buf, typed_base, m.bytes);
    if (count == 0 || m.t->size == 0) return MPI_SUCCESS;
    std::vector<char> packed((size_t)m.t->size * count);
    Dtype* t = const_cast<Dtype*>(m.t);
    size_t p = 0;
    auto run = [&](int64_t i, int64_t disp, int64_t len) {
        memcpy(packed.data() + p, typed_base + i * t->extent + disp, (size_t)len);
        p += (size_t)len;
    };
    for (size_t i = 0; i < count; ++i)
        dtype_for_each_run(t, [&](int64_t disp, int64_t len) { run((int64_t)i, disp, len); });
    return dt_unpack_any(t, (int64_t)count, packed.data(), buf);
}

// inout = in (op) inout over `count` elements, typed bases
void img_call(const OpRef& op, MPI_Datatype dt, const Img& m, size_t count, const char* in, char* io)
{
    MPI_Datatype d = dt;
    if (m.t) {
        int len = (int)count;      // API counts are int
        op.user_fn(const_cast<char*>(in), io, &len, &d);
        return;
    }
    for (size_t off = 0; off < count;) {
        size_t n = std::min(count - off, (size_t)0x7fffffff);
        int len = (int)n;
        op.user_fn(const_cast<char*>(in) + off * m.esz, io + off * m.esz, &len, &d);
        off += n;
    }
}

// The host executor of a combine plan (userop_plan, msx_schedule.cpp), the
// whole host user-op path: every rank's image of the `total` elements at `src`
// is gathered into one flat buffer; the plan's steps then run in place over
// the p images -- over elements [first, first + count) of each -- and
// out_count elements from element out_first of the result block go to
// recvbuf.  plan == nullptr: a rank that only contributes (not the root of a
// reduce, or no elements of its own).
int host_user_run(Comm* c, const void* src, void* recvbuf, size_t total, MPI_Datatype dt, const OpRef& op,
                  const CombinePlan* plan, size_t first, size_t count, size_t out_first, size_t out_count)
{
    const Img mf = img_of(dt, total);
    std::vector<char> mine(mf.bytes), all((size_t)c->size * mf.bytes);
    int rc = img_load(mf, src, mine.data());
    if (rc == MPI_SUCCESS) rc = c->tp->allgather(mine.data(), mf.bytes, all.data());
    if (rc != MPI_SUCCESS || !plan) return rc;
    const int64_t unit = mf.t ? mf.t->extent : (int64_t)mf.esz;
    // typed base of element `el` of rank r's contribution
    auto at = [&](int r, size_t el) { return all.data() + (size_t)r * mf.bytes - mf.lo + (int64_t)el * unit; };
    const Img mc = img_of(dt, count);
    for (const CombineStep& s : plan->steps) img_call(op, dt, mc, count, at(s.in, first), at(s.io, first));
    if (plan->result < 0 || out_count == 0) return MPI_SUCCESS;     // rank 0 of an exscan: recvbuf untouched
    return img_store(img_of(dt, out_count), out_count, at(plan->result, out_first), recvbuf);
}

// The reference's recursive-doubling order (reduce.cpp:3890-3925,
// non-commutative branch included) with the user's function.
int host_user_allreduce(Comm* c, const void* sendbuf, void* recvbuf, size_t count,
                        MPI_Datatype dt, const OpRef& op)
{
    const CombinePlan plan = userop_plan(UserColl::allreduce, c->size, c->rank, op.commutative, false, count, 0);
    return host_user_run(c, sendbuf == MPI_IN_PLACE ? recvbuf : sendbuf, recvbuf, count, dt, op, &plan, 0, count, 0,
                         count);
}

// Engine-private device scratch (grows, never shrinks; engine worker only).
char* dev_scratch(size_t bytes)
{
    static char* p = nullptr;
    static size_t cap = 0;
    if (bytes > cap) {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        if (hipMalloc(reinterpret_cast<void**>(&p), bytes) != hipSuccess) return nullptr;
        cap = bytes;
    }
    return p;
}

// ---- window collectives (push model) ----------------------------------------
// Every rank owns one IPC-mapped device window of 2*C bytes: an IN area of p
// sub-slots of Q = C/p bytes (sub-slot k receives rank k's contribution) and an
// OUT area of C bytes (the reduced chunk, assembled from every owner's piece).
// User buffers are never IPC-mapped (ROCm 7.2 hangs opening handles of
// allocations > 2 GiB, and user memory may be host memory).  Data crosses
// xGMI only as REMOTE WRITES (posted stores, all peer links at once);
// reductions read local HBM only:
//   scatter : piece r of my chunk -> IN(r)[sub-slot me]             (xGMI writes)
//   barrier A (every contribution landed: writers synced before it)
//   reduce  : my piece from IN(me)[0..p-1], the reference's expression tree
//             per element -> OUT(me)[my piece]                        (local)
//   push    : OUT(me)[my piece] -> OUT(r)[my piece], every r          (xGMI writes)
//   barrier B (every piece landed)
//   collect : OUT(me) -> recvbuf                                      (local / D2H)
// One slot suffices: a peer scatters chunk i+1 into IN(me) only after barrier B
// of chunk i (I finished reading IN(me) before it) and pushes into OUT(me)
// only after barrier A of chunk i+1 (I collected chunk i before it).  After a
// collective's last barrier B no peer touches my window, so the next
// collective needs no extra barrier.
// Default C = 960 MiB, the largest whose window (2 C + flags) stays below the
// 2 GiB IPC mapping limit: 1.9 GB of each rank's 288 GB.  Rounds 1-4 used
// 512 MiB; with the larger window c3 takes 3 pipelined chunks instead of 5 at
// p = 8, and 2 ranks on one MI355X measured c3 1.87 -> 1.77 ms and c4 3.80 ->
// 3.60 ms (bench.py's engine-variant sweep, profiles/r04/bench_n2_variants.json).
size_t chunk_bytes()
{
    static size_t c = [] {
        size_t v = (size_t)960 << 20;
        if (const char* e = getenv("MSX_CHUNK_BYTES")) v = (size_t)atoll(e);
        if (v < ((size_t)1 << 16)) v = (size_t)1 << 16;
        if (v > ((size_t)960 << 20)) v = (size_t)960 << 20;   // whole window < 2 GiB (IPC limit)
        return v & ~(size_t)4095;
    }();
    return c;
}

namespace {
// Arrival flags of the barrier-free allreduce live behind the two areas:
// flag k of window r (8 bytes) = the last call sequence rank k posted to r.
constexpr size_t kFlagBytes = 64 << 10;
}  // namespace

// Passive-target RMA staging (its own IPC allocation, created by the first
// passive-target window of a communicator): p payload slots (written by each
// origin) then p fetch slots (written by each target), the agreed size / (2p) each.
// Every slot-sized piece of a lock / PSCW operation costs one host handshake
// with the target's service thread (~50 us), so the area is sized for large
// pieces (MSX_RMA_BYTES, default 512 MiB), below the 2 GiB IPC limit.  256 MiB lock / PSCW accumulates, 2 ranks on one MI355X
// (profiles/r02/rma_area_*.json): 1.27 ms with 64 MiB, 0.66 ms with 256 MiB,
// 0.53 ms with 512 MiB (= the fence epoch's 0.54 ms).
// The area belongs to the communicator's transport: every communicator with a
// window holds one per rank.  Without MSX_RMA_BYTES the default is capped per
// GPU: 512 MiB divided by the ranks that share this GPU (8 ranks on one GPU:
// 64 MiB each), at least 64 MiB.  `share` is counted by the transport from
// every rank's PCI bus id, and the ranks then take the minimum of their sizes
// (IpcTransport::rma_window), so all of them address the same slots.
size_t rma_bytes_for(int share)
{
    size_t b = (size_t)512 << 20;
    if (share > 1) b = std::max(b / (size_t)share, (size_t)64 << 20);
    if (const char* e = getenv("MSX_RMA_BYTES")) b = (size_t)atoll(e);
    const size_t cap = ((size_t)2 << 30) - ((size_t)1 << 20);      // IPC mapping limit
    b = std::min(b, cap);
    return std::max(b, (size_t)4 << 20) & ~(size_t)4095;
}

// Sub-slots are Q bytes long but S = Q + skew apart: the p-source tree reads
// every sub-slot at the same offset, and sources a power of two apart lose
// HBM bandwidth to channel aliasing (scripts/tree_skew_probe.py on MI355X,
// profiles/r01/tree_skew_probe.log: 8 x 32 MiB, 6.27 TB/s at a 32 MiB stride,
// 6.51-6.56 TB/s with 4-68 KiB added).
size_t sub_skew(size_t per_rank)
{
    if (per_rank >= ((size_t)16 << 20)) return (size_t)68 << 10;
    return (per_rank / 16) & ~(size_t)255;
}

// usable bytes of one sub-slot of a window with chunk C over p ranks: C/p
// minus the skew, so the IN area is exactly C.  (Late round 3 tried the whole
// C/p with the skew on top and reverted it; round 4 re-ran that layout to
// rule it out for the wrong results DESIGN.md §2 explains.)
size_t sub_len(size_t C, int p)
{
    const size_t per = C / (size_t)p;
    return (per - sub_skew(per)) & ~(size_t)255;
}

// Half an IN sub-slot for p ranks, whole 256-byte lines: what one GPU-flag
// call, chunk or round may write into a peer's sub-slot while the other half
// is still being read.
size_t half_bytes(int p) { return (sub_len(chunk_bytes(), p) / 2) & ~(size_t)255; }

namespace {
// IN area of a window: p sub-slots sub_skew apart, C bytes in all
size_t in_bytes(size_t C, int /*p*/) { return C; }
}  // namespace

// Largest message (bytes) of the barrier-free two-step allreduce / reduce
// (MSX_TWO_STEP_MAX; 0 = always the host-barrier schedule).  By default every
// Rabenseifner-sized message takes it, longer ones as a GPU-synchronised
// pipeline of window-half chunks (round 4; rounds 1-3 stopped at 256 MiB and
// ran the rest through host barriers, five host syncs per chunk).  2 ranks on
// one MI355X (scripts/allreduce_probe.sh, profiles/r02/two_step_*) measured
// 1 MiB 62.6 -> 28.5 us, 4 MiB 64.3 -> 32.5, 16 MiB 75.6 -> 45.8,
// 64 MiB 154.8 -> 133.0, 128 MiB 265 -> 249; 4 ranks 64 MiB 310 -> 254.
// Defaults (round 5; same value on every rank, gpu_shared is agreed):
//  * ranks sharing a GPU: 0, the host-barrier schedules (round 4's default
//    there; the flag schedules run when MSX_TWO_STEP_MAX asks, as the tests
//    do).  The wrong results recorded on this path in rounds 3-4 were the test
//    harness's own pageable transfers, not the schedule.
//  * one rank per GPU: 256 MiB, the rounds 1-3 cap -- a single chunk of the
//    two-step schedule; longer messages run the host-barrier pipeline.  The
//    cross-GPU data plane has not run on hardware yet (no multi-GPU box has
//    been available to the tests), so the multi-chunk GPU-flag pipeline is
//    opt-in (MSX_TWO_STEP_MAX) until the one-rank-per-GPU suites pass.
size_t two_step_max(const Transport* tp)
{
    static const char* e = getenv("MSX_TWO_STEP_MAX");
    if (e) return (size_t)atoll(e);
    return tp->gpu_shared ? 0 : (size_t)256 << 20;
}

// Pinned bounce buffers of the engine (engine worker, or the one inline
// blocking call): 0 = this rank's contribution, 1 = the result.
Bounce& engine_bounce(int i)
{
    static Bounce b[2];
    return b[i];
}

// Pinned host word the arrival wait reports a timeout through (engine worker
// only); returns its device view.
int* wait_err_word(int** host)
{
    static int* h = nullptr;
    static int* d = nullptr;
    if (!h) {
        if (hipHostMalloc(reinterpret_cast<void**>(&h), sizeof(int), hipHostMallocCoherent | hipHostMallocMapped) !=
            hipSuccess) {
            h = nullptr;
            return nullptr;
        }
        if (hipHostGetDevicePointer(reinterpret_cast<void**>(&d), h, 0) != hipSuccess) d = h;
    }
    *host = h;
    return d;
}

int get_windows(Transport* tp, Windows* w, bool rd_single)
{
    w->C = chunk_bytes();
    w->Q = sub_len(w->C, tp->size);
    w->S = w->Q + sub_skew(w->C / (size_t)tp->size);
    w->I = in_bytes(w->C, tp->size);
    // [IN: p sub-slots, C bytes][OUT: C][flags]: 2 C + 64 KiB, below the
    // 2 GiB IPC mapping limit for C <= 960 MiB (checked: a larger allocation
    // would hang hipIpcOpenMemHandle, see map_peers)
    if (w->I + w->C + kFlagBytes > ((size_t)2046 << 20)) {
        set_error("window of %zu bytes exceeds the IPC mapping limit (MSX_CHUNK_BYTES too large)",
                  w->I + w->C + kFlagBytes);
        return MPI_ERR_INTERN;
    }
    int rc = tp->window(w->I + w->C + kFlagBytes, w->base);
    if (rc == MPI_SUCCESS && tp->window_open && !rd_single) {
        // the last recursive-doubling call left without its closing barrier:
        // peers may still be reading their IN areas
        rc = tp->barrier();
        tp->window_open = false;
    }
    if (!rd_single) tp->out_quiet = false;      // a host-barrier user of the OUT areas
    return rc;
}

namespace {
// Copies of at least kKernelCopyMin bytes within this GPU's memory (HBM
// buffers, its own window) run on the engine's copy kernel: 256 MiB local
// copies take 68 us there and 99 us as hipMemcpyAsync's blit
// (profiles/r02/copy/copy_cmp.log).  Host memory keeps hipMemcpyAsync (DMA).
constexpr size_t kKernelCopyMin = (size_t)1 << 20;
}  // namespace

int copy_async(void* dst, const void* src, size_t bytes, hipStream_t s)
{
    if (!bytes) return MPI_SUCCESS;
    if (bytes >= kKernelCopyMin) {
        const BufInfo bs = classify(src), bd = classify(dst);
        int cur = -1;
        (void)hipGetDevice(&cur);
        // both on this GPU (a peer's window or another GPU's buffer: the blit),
        // 16-byte aligned (otherwise the kernel falls back to one byte per
        // lane, far below the blit)
        if (bs.place == Place::Device && bd.place == Place::Device && bs.device == cur && bd.device == cur &&
            (((uintptr_t)bs.dev | (uintptr_t)bd.dev) & 15) == 0) {
            const void* ps = bs.dev;
            void* pd = bd.dev;
            hipError_t e = launch_copy_segs(&ps, &pd, &bytes, 1, s);
            return e == hipSuccess ? MPI_SUCCESS : hip_fail(e, "copy kernel");
        }
    }
    // a pageable host side never goes to HIP's copy path (xfer_sync)
    if (host_pageable(dst) || host_pageable(src)) return xfer_sync(dst, src, bytes, s);
    hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, s);   // xfer: device/pinned
    return e == hipSuccess ? MPI_SUCCESS : hip_fail(e, "stage copy");
}

EngineStats g_stats;

// The communicator's second engine stream: local copies that overlap xGMI
// work.  Created on first use; nullptr (callers then stay on their stream)
// if HIP refuses.
hipStream_t aux_stream(Transport* tp)
{
    if (!tp->aux && hipStreamCreateWithFlags(&tp->aux, hipStreamNonBlocking) != hipSuccess) {
        (void)hipGetLastError();
        tp->aux = nullptr;
    }
    return tp->aux;
}

// Device view of `len` bytes of a user buffer at byte offset `off`: the buffer
// itself when it is device memory, else staged into `stage` (H2D).
int device_view(const BufInfo& b, const char* user, size_t off, size_t len, char* stage,
                hipStream_t s, const char** out)
{
    if (b.place == Place::Device) {
        *out = static_cast<const char*>(b.dev) + off;
        return MPI_SUCCESS;
    }
    *out = stage;
    return copy_async(stage, user + off, len, s);
}

int engine_stats(double* out, int n, int reset)
{
    return worker().submit([out, n, reset]() -> int {
        const double v[8] = {g_stats.t[0], g_stats.t[1], g_stats.t[2], g_stats.t[3], g_stats.t[4],
                             (double)g_stats.chunks, (double)g_stats.calls, (double)g_stats.flag_calls};
        for (int i = 0; i < n && i < 8; ++i) out[i] = v[i];
        if (reset) g_stats = EngineStats();
        return 8;
    }).get();
}

// Link roofline probe: every rank writes `bytes` from its own window into
// its sub-slot of EVERY peer's IN area at once (the scatter step's traffic
// pattern: p-1 concurrent remote-write streams per GPU, all xGMI links busy),
// `reps` times.  *seconds = median time of one all-peer write of *used
// bytes per peer (the request capped at one window sub-slot).  The result is
// the measured per-GPU outbound bandwidth that the collectives' busBW is
// judged against (confirm the link figures by measurement).
int engine_peer_write_probe(Comm* c, size_t bytes, int reps, double* seconds, int64_t* used)
{
    *used = 0;
    if (!c->tp || c->size == 1) {
        *seconds = 0;
        return MPI_SUCCESS;
    }
    int rc = ensure_device();
    if (rc != MPI_SUCCESS) return rc;
    return worker().submit([c, bytes, reps, seconds, used]() -> int {
        Transport* tp = c->tp;
        const int p = c->size, me = c->rank;
        Windows w;
        int rc = get_windows(tp, &w);
        if (rc != MPI_SUCCESS) return rc;
        const size_t n = std::min(bytes, w.Q) & ~(size_t)255;
        *used = (int64_t)n;
        hipStream_t s = tp->stream();
        std::vector<double> ts;
        for (int it = 0; it <= reps && rc == MPI_SUCCESS; ++it) {
            Segs sg;
            for (int r = 0; r < p; ++r)
                if (r != me) sg.add(w.out(me), w.sub(r, me), n);
            rc = tp->barrier();
            const double t0 = now_s();
            if (rc == MPI_SUCCESS) rc = sg.run(s, "peer write probe");
            if (rc == MPI_SUCCESS) rc = sync_stream(s, "peer write probe");
            const double t1 = now_s();
            if (rc == MPI_SUCCESS) rc = tp->barrier();
            if (it > 0) ts.push_back(t1 - t0);       // the first is a warm-up
        }
        if (rc == MPI_SUCCESS && !ts.empty()) {
            std::sort(ts.begin(), ts.end());
            *seconds = ts[ts.size() / 2];
        }
        return rc;
    }).get();
}

std::shared_future<int> engine_async(std::function<int()> fn) { return worker().submit(std::move(fn)); }

}  // namespace msx
