// msx_api_rma.cpp — the one-sided API: MPI_Alloc_mem / MPI_Free_mem, windows and
// their table, fence, passive-target and post-start-complete-wait
// synchronisation, data movement and its request-based forms.
#include <algorithm>
#include <atomic>
#include <map>
#include <mutex>
#include <stdlib.h>
#include <vector>

#include "msx_api.h"
#include "msx_dtype.h"
#include "msx_transport.h"

using namespace msx;

// ===========================================================================
// one-sided communication (api/mpi_win.cpp, api/mpi_rma.cpp), fence epochs
// ===========================================================================
namespace {

std::mutex g_win_mu;
std::vector<RmaWin*> g_wins;          // direct handles 0xA0000000 | index
constexpr int kWinKindBits = 0xA0000000;

// MpiaWinValidateHandle
int v_win(MPI_Win h, RmaWin** out)
{
    *out = nullptr;
    if (h == MPI_WIN_NULL) { set_error("null window"); return MPI_ERR_WIN; }
    std::lock_guard<std::mutex> g(g_win_mu);
    const unsigned idx = (unsigned)h & 0x03ffffffu;
    if (((unsigned)h & 0xfc000000u) != (unsigned)kWinKindBits || idx >= g_wins.size() || !g_wins[idx]) {
        set_error("invalid window 0x%x", h);
        return MPI_ERR_WIN;
    }
    *out = g_wins[idx];
    return MPI_SUCCESS;
}

int err_win(RmaWin* w, const char* fn, int code)
{
    if (code == MPI_SUCCESS) return code;
    // MPIR_Err_return_win (mpid/error.cpp:142-151): a window without an
    // error handler of its own reports through MPI_COMM_WORLD's
    if (!w || w->errhandler == MPI_ERRHANDLER_NULL) return err_return(nullptr, fn, code);
    return err_return_h(w->errhandler, fn, code);
}

// target datatype checks (MpiaDatatypeValidate with MPI_IN_PLACE as buffer),
// the displacement and the rank, in the order of mpi_rma.cpp:697-735
int v_target(RmaWin* w, int target_count, MPI_Datatype target_dt, int target_rank, MPI_Aint target_disp)
{
    int rc = v_dtype_any(MPI_IN_PLACE, target_count, target_dt);
    if (rc != MPI_SUCCESS) return rc;
    if (target_disp < 0) { set_error("negative target displacement"); return MPI_ERR_DISP; }
    if (target_rank != MPI_PROC_NULL && (target_rank < 0 || target_rank >= w->comm->size)) {
        set_error("invalid target rank %d", target_rank);
        return MPI_ERR_RANK;
    }
    return MPI_SUCCESS;
}

// Origin and target must describe the same data: predefined pairs the same
// type and count; with a derived type on either side the same number of bytes
// of the same basic element type (the type signatures of MPI-2.2 §11.3).
int v_match(int ocount, MPI_Datatype odt, int tcount, MPI_Datatype tdt)
{
    if (!dtype_is_derived(odt) && !dtype_is_derived(tdt)) {
        if (odt != tdt) { set_error("origin and target datatypes differ (0x%x, 0x%x)", odt, tdt); return MPI_ERR_TYPE; }
        if (ocount != tcount) { set_error("origin and target counts differ (%d, %d)", ocount, tcount); return MPI_ERR_COUNT; }
        return MPI_SUCCESS;
    }
    const Dtype* o = dtype_lookup(odt);
    const Dtype* t = dtype_lookup(tdt);
    if ((int64_t)ocount * o->size != (int64_t)tcount * t->size) {
        set_error("origin and target describe %lld and %lld bytes", (long long)((int64_t)ocount * o->size),
                  (long long)((int64_t)tcount * t->size));
        return MPI_ERR_TYPE;
    }
    if (o->eltype != t->eltype && o->size > 0) {
        set_error("origin and target element types differ (0x%x, 0x%x)", o->eltype, t->eltype);
        return MPI_ERR_TYPE;
    }
    return MPI_SUCCESS;
}

// Device temporary holding `count` instances of `dt` from `src`, packed.
int pack_to_device(const void* src, int64_t count, MPI_Datatype dt, void** out)
{
    *out = nullptr;
    const Dtype* t = dtype_lookup(dt);
    const size_t bytes = (size_t)(count * t->size);
    if (bytes == 0) return MPI_SUCCESS;
    int rc = ensure_device();
    if (rc != MPI_SUCCESS) return rc;
    if (hipMalloc(out, bytes) != hipSuccess) { *out = nullptr; set_error("rma temporary"); return MPI_ERR_NO_MEM; }
    rc = dt_pack_any(t, count, src, *out);
    if (rc != MPI_SUCCESS) { (void)hipFree(*out); *out = nullptr; }
    return rc;
}

// Queue a remote operation, or apply it now when the target is this rank
// (win.cpp:1570-1590: MPIDI_Win_local_accumulate / MPIR_Localcopy).
// Derived origin / result types are packed / unpacked on the origin's GPU; a
// derived target type travels as its flattened layout.
int rma_issue(RmaWin* w, RmaKind kind, int target, MPI_Aint disp, int opidx, const void* origin, int ocount,
              MPI_Datatype odt, void* result, int rcount, MPI_Datatype rdt, int tcount, MPI_Datatype tdt,
              const void* compare)
{
    RmaDesc d;
    d.kind = kind;
    d.target = target;
    d.opidx = opidx;
    d.tdisp = (int64_t)disp * w->disp_units[(size_t)target];    // the TARGET's disp_unit
    const bool self = target == w->comm->rank;
    const Dtype* T = nullptr;
    if (dtype_is_derived(tdt)) {
        T = dtype_lookup(tdt);
        d.dt = T->eltype;
        d.count = tcount;
        d.usize = T->size;
        d.uext = T->extent;
        dt_span(T, tcount, &d.span_lo, &d.span_hi);
        if (T->size == 0) return MPI_SUCCESS;
        if (!self) {
            d.layout = (int32_t)w->blob.size();
            dtype_serialize(T, w->blob);
        }
    } else {
        d.dt = tdt;
        d.count = tcount;
        d.usize = d.uext = type_size(tdt);
    }
    RmaLocal l;
    l.origin = origin;
    l.result = result;
    l.compare = compare;
    int rc = MPI_SUCCESS;
    const bool sends = kind == RMA_PUT || ((kind == RMA_ACC || kind == RMA_GACC) && opidx != O_NOOP);
    const bool fetches = kind == RMA_GET || kind == RMA_GACC;
    // the typed kernels read the payload and write fetched bytes in device memory
    if (sends && (dtype_is_derived(odt) || (T && classify(origin).place != Place::Device))) {
        rc = pack_to_device(origin, ocount, odt, &l.tmp_origin);
        l.origin = l.tmp_origin;
    }
    if (rc == MPI_SUCCESS && fetches && (dtype_is_derived(rdt) || (T && classify(result).place != Place::Device))) {
        const size_t bytes = (size_t)(rcount * dtype_lookup(rdt)->size);
        if (bytes && hipMalloc(&l.tmp_result, bytes) != hipSuccess) {
            l.tmp_result = nullptr;
            set_error("rma temporary");
            rc = MPI_ERR_NO_MEM;
        }
        l.result = l.tmp_result;
        l.result_user = result;
        l.result_dt = rdt;
        l.result_count = rcount;
        if (l.tmp_result) dtype_add_ref(rdt);      // released by rma_local_complete
    }
    if (rc != MPI_SUCCESS) {
        rma_local_complete(l);
        return rc;
    }
    if (self) {
        engine_rma_self_guard(w, true);      // not concurrently with the window's service thread
        rc = rma_apply_self(w, d, l, T);
        engine_rma_self_guard(w, false);
        const int r2 = rma_local_complete(l);
        return rc != MPI_SUCCESS ? rc : r2;
    }
    w->q.push_back(d);
    w->ql.push_back(l);
    return MPI_SUCCESS;
}

int rma_op(MPI_Op op, OpRef* r, bool allow_noop)
{
    int rc = v_op_handle(op, r);       // MpiaOpValidate(rmaOp = true): handle only
    if (rc != MPI_SUCCESS) return rc;
    if (!allow_noop && r->opidx == O_NOOP) { set_error("MPI_NO_OP not allowed"); return MPI_ERR_OP; }
    if ((rc = v_no_sum_wide(*r, "one-sided calls")) != MPI_SUCCESS) return rc;
    if (r->opidx == O_NULL) {
        // do_accumulate_op: **opnotpredefined (packethandling.cpp:2934-2937)
        set_error("user-defined operations are not allowed in RMA");
        return MPI_ERR_OP;
    }
    return MPI_SUCCESS;
}

}  // namespace

// ---- MPI_Alloc_mem / MPI_Free_mem (api/mpi_env.cpp:841-945) ---------------------
// The reference returns heap memory (MPID_Alloc_mem, mpid/env.cpp:1745).  Here
// it is pinned host memory when a GPU is present: still ordinary CPU memory,
// and the combine kernels read and write it in place over PCIe (the zero-copy
// host path), instead of staging pageable pages.
namespace {
std::mutex g_mem_mu;
std::map<void*, bool> g_mem;          // base -> pinned (hipHostMalloc) or heap

int alloc_mem(MPI_Aint size, void** out)
{
    const size_t n = size > 0 ? (size_t)size : 1;
    void* p = nullptr;
    bool pinned = false;
    if (device_count_noinit() > 0 && ensure_device() == MPI_SUCCESS &&
        hipHostMalloc(&p, n, hipHostMallocDefault) == hipSuccess) {
        pinned = true;
    } else {
        (void)hipGetLastError();
        p = malloc(n);
    }
    if (!p) { set_error("MPI_Alloc_mem: %lld bytes not available (**allocmem)", (long long)size); return MPI_ERR_NO_MEM; }
    std::lock_guard<std::mutex> g(g_mem_mu);
    g_mem[p] = pinned;
    *out = p;
    return MPI_SUCCESS;
}

int free_mem(void* base)
{
    bool pinned;
    {
        std::lock_guard<std::mutex> g(g_mem_mu);
        auto it = g_mem.find(base);
        if (it == g_mem.end()) { set_error("memory %p was not allocated by MPI_Alloc_mem", base); return MPI_ERR_BASE; }
        pinned = it->second;
        g_mem.erase(it);
    }
    if (pinned) (void)hipHostFree(base);
    else free(base);
    return MPI_SUCCESS;
}
}  // namespace

MSX_EXPORT int MPI_Alloc_mem(MPI_Aint size, MPI_Info info, void* baseptr)
{
    MSX_REQUIRE_INIT("MPI_Alloc_mem");
    int rc = MPI_SUCCESS;
    if (size < 0) { set_error("negative size %lld (**argneg)", (long long)size); rc = MPI_ERR_ARG; }
    else if (!baseptr) { set_error("null baseptr"); rc = MPI_ERR_ARG; }
    else if (info != MPI_INFO_NULL) { set_error("only MPI_INFO_NULL is supported"); rc = MPI_ERR_INFO; }
    void* p = nullptr;
    if (rc == MPI_SUCCESS) rc = alloc_mem(size, &p);
    if (rc == MPI_SUCCESS) *static_cast<void**>(baseptr) = p;
    return err_return(nullptr, "MPI_Alloc_mem", rc);
}

// mpi_env.cpp:920-945: errors are returned, not raised through a handler
MSX_EXPORT int MPI_Free_mem(void* base)
{
    MSX_REQUIRE_INIT("MPI_Free_mem");
    if (!base) { set_error("null base"); return MPI_ERR_BASE; }
    return free_mem(base);
}

MSX_EXPORT int MPI_Win_create(void* base, MPI_Aint size, int disp_unit, MPI_Info info, MPI_Comm comm,
                              MPI_Win* win)
{
    MSX_REQUIRE_INIT("MPI_Win_create");
    Comm* c;
    int rc = v_intracomm(comm, &c);
    if (rc == MPI_SUCCESS && info != MPI_INFO_NULL) { set_error("only MPI_INFO_NULL is supported"); rc = MPI_ERR_INFO; }
    if (rc == MPI_SUCCESS && size < 0) { set_error("negative window size"); rc = MPI_ERR_SIZE; }
    if (rc == MPI_SUCCESS && disp_unit <= 0) { set_error("disp_unit must be positive"); rc = MPI_ERR_ARG; }
    if (rc == MPI_SUCCESS && win == nullptr) { set_error("null win"); rc = MPI_ERR_ARG; }
    if (rc != MPI_SUCCESS) return err_return(c, "MPI_Win_create", rc);
    auto* w = new RmaWin();
    w->comm = c;
    w->base = static_cast<char*>(base);
    w->size = size;
    w->disp_unit = disp_unit;
    w->lock_mode.assign((size_t)c->size, 0);
    w->lock_held.assign((size_t)c->size, 0);
    rc = engine_rma_create(w);
    if (rc != MPI_SUCCESS) {
        delete w;
        return err_return(c, "MPI_Win_create", rc);
    }
    std::lock_guard<std::mutex> g(g_win_mu);
    size_t idx = 0;
    while (idx < g_wins.size() && g_wins[idx]) ++idx;
    if (idx == g_wins.size()) g_wins.push_back(nullptr);
    g_wins[idx] = w;
    w->handle = kWinKindBits | (int)idx;
    *win = w->handle;
    return MPI_SUCCESS;
}

// MPI_Win_allocate (api/mpi_win.cpp:295-380): MPI_Alloc_mem + MPI_Win_create,
// the memory freed by MPI_Win_free
MSX_EXPORT int MPI_Win_allocate(MPI_Aint size, int disp_unit, MPI_Info info, MPI_Comm comm, void* baseptr,
                                MPI_Win* win)
{
    MSX_REQUIRE_INIT("MPI_Win_allocate");
    Comm* c;
    int rc = v_intracomm(comm, &c);
    if (rc == MPI_SUCCESS && info != MPI_INFO_NULL) { set_error("only MPI_INFO_NULL is supported"); rc = MPI_ERR_INFO; }
    if (rc == MPI_SUCCESS && size < 0) { set_error("negative window size (**rmasize)"); rc = MPI_ERR_SIZE; }
    if (rc == MPI_SUCCESS && disp_unit <= 0) { set_error("disp_unit must be positive"); rc = MPI_ERR_ARG; }
    if (rc == MPI_SUCCESS && (win == nullptr || baseptr == nullptr)) { set_error("null win / baseptr"); rc = MPI_ERR_ARG; }
    void* p = nullptr;
    if (rc == MPI_SUCCESS) rc = alloc_mem(size, &p);
    if (rc != MPI_SUCCESS) return err_return(c, "MPI_Win_allocate", rc);
    rc = MPI_Win_create(p, size, disp_unit, info, comm, win);
    if (rc != MPI_SUCCESS) {
        (void)free_mem(p);
        return rc;                    // already reported by MPI_Win_create
    }
    RmaWin* w;
    (void)v_win(*win, &w);
    w->owned = p;
    *static_cast<void**>(baseptr) = p;
    return MPI_SUCCESS;
}

MSX_EXPORT int MPI_Win_free(MPI_Win* win)
{
    MSX_REQUIRE_INIT("MPI_Win_free");
    if (!win) { set_error("null win"); return err_return(nullptr, "MPI_Win_free", MPI_ERR_ARG); }
    RmaWin* w;
    int rc = v_win(*win, &w);
    if (rc != MPI_SUCCESS) return err_win(nullptr, "MPI_Win_free", rc);
    if (!w->q.empty()) { set_error("MPI_Win_free with operations pending (no closing fence)"); return err_win(w, "MPI_Win_free", MPI_ERR_RMA_SYNC); }
    for (int m : w->lock_mode)
        if (m) { set_error("MPI_Win_free inside a passive-target epoch"); return err_win(w, "MPI_Win_free", MPI_ERR_RMA_SYNC); }
    if (w->access_epoch || w->exposure_epoch) {
        set_error("MPI_Win_free inside a post-start-complete-wait epoch");
        return err_win(w, "MPI_Win_free", MPI_ERR_RMA_SYNC);
    }
    rc = coll_barrier(w->comm);       // every rank is done with the window
    if (rc != MPI_SUCCESS) return err_win(w, "MPI_Win_free", rc);
    engine_rma_free(w);               // no request can be in flight after the barrier
    if (w->owned) (void)free_mem(w->owned);
    {
        std::lock_guard<std::mutex> g(g_win_mu);
        g_wins[(size_t)(*win & 0x03ffffff)] = nullptr;
    }
    delete w;
    *win = MPI_WIN_NULL;
    return MPI_SUCCESS;
}

MSX_EXPORT int MPI_Win_fence(int assert_, MPI_Win win)
{
    MSX_REQUIRE_INIT("MPI_Win_fence");
    RmaWin* w;
    int rc = v_win(win, &w);
    if (rc != MPI_SUCCESS) return err_win(nullptr, "MPI_Win_fence", rc);
    (void)assert_;                    // hints only
    return err_win(w, "MPI_Win_fence", engine_rma_fence(w));
}

// ---- passive target (api/mpi_win.cpp:1153-1990, mpid/win.cpp:4090-4500) ----------
namespace {
// MpiaCommValidateSendRank: a rank of the window's group or MPI_PROC_NULL
int v_lock_rank(RmaWin* w, int rank)
{
    if (rank == MPI_PROC_NULL || (rank >= 0 && rank < w->comm->size)) return MPI_SUCCESS;
    set_error("invalid rank %d", rank);
    return MPI_ERR_RANK;
}

// MPID_Win_lock: a lock on this rank itself is acquired now (blocking); on
// another rank it is requested lazily, granted at the first flush / unlock
int win_lock(RmaWin* w, int lock_type, int rank, int assert_)
{
    (void)assert_;                    // MPI_MODE_NOCHECK: a hint
    if (rank == MPI_PROC_NULL) return MPI_SUCCESS;
    if (w->lock_mode[(size_t)rank]) {
        set_error("rank %d is already locked in this window (**rmasyncq)", rank);
        return MPI_ERR_OTHER;
    }
    if (rank == w->comm->rank) {
        const int rc = engine_rma_lock(w, rank, lock_type);
        if (rc != MPI_SUCCESS) return rc;
        w->lock_held[(size_t)rank] = 1;
    }
    w->lock_mode[(size_t)rank] = lock_type;
    return MPI_SUCCESS;
}

int win_unlock(RmaWin* w, int rank)
{
    if (rank == MPI_PROC_NULL) return MPI_SUCCESS;
    if (!w->lock_mode[(size_t)rank]) {
        set_error("MPI_Win_unlock without MPI_Win_lock on rank %d (**rmasync)", rank);
        return MPI_ERR_OTHER;
    }
    const int rc = engine_rma_flush(w, rank);
    engine_rma_unlock_target(w, rank);
    w->lock_mode[(size_t)rank] = 0;
    w->lock_held[(size_t)rank] = 0;
    return rc;
}
}  // namespace

MSX_EXPORT int MPI_Win_lock(int lock_type, int rank, int assert_, MPI_Win win)
{
    MSX_REQUIRE_INIT("MPI_Win_lock");
    RmaWin* w;
    int rc = v_win(win, &w);
    if (rc != MPI_SUCCESS) return err_win(nullptr, "MPI_Win_lock", rc);
    if (lock_type != MPI_LOCK_SHARED && lock_type != MPI_LOCK_EXCLUSIVE) {
        set_error("invalid lock type %d (**locktype)", lock_type);
        rc = MPI_ERR_OTHER;
    }
    if (rc == MPI_SUCCESS) rc = v_lock_rank(w, rank);
    if (rc == MPI_SUCCESS) rc = win_lock(w, lock_type, rank, assert_);
    return err_win(w, "MPI_Win_lock", rc);
}

MSX_EXPORT int MPI_Win_unlock(int rank, MPI_Win win)
{
    MSX_REQUIRE_INIT("MPI_Win_unlock");
    RmaWin* w;
    int rc = v_win(win, &w);
    if (rc != MPI_SUCCESS) return err_win(nullptr, "MPI_Win_unlock", rc);
    rc = v_lock_rank(w, rank);
    if (rc == MPI_SUCCESS) rc = win_unlock(w, rank);
    return err_win(w, "MPI_Win_unlock", rc);
}

// ---- post-start-complete-wait (api/mpi_win.cpp:28-70,979-1030,1331-1381,
// 1487-1537,1566-1613,1769-1808; mpid/win.cpp:2001-2012,3689-4088) -------------
namespace {
// The window ranks of a group's members (MpiaGroupValidateHandle, then
// MPIR_Group_translate_ranks into the window's communicator).  A member outside
// the window's communicator is an invalid group here (the reference would
// address rank MPI_UNDEFINED).
int group_window_ranks(RmaWin* w, MPI_Group g, std::vector<int>* ranks)
{
    std::vector<int> lp;
    int rc = group_members(g, &lp);
    if (rc != MPI_SUCCESS) return rc;
    ranks->clear();
    for (int id : lp) {
        const auto& cl = w->comm->lpid;
        const auto it = std::find(cl.begin(), cl.end(), id);
        if (it == cl.end()) {
            set_error("group member (process %d) is not in the window's communicator", id);
            return MPI_ERR_GROUP;
        }
        ranks->push_back((int)(it - cl.begin()));
    }
    return MPI_SUCCESS;
}
void pscw_sizes(RmaWin* w)
{
    const size_t p = (size_t)w->comm->size;
    if (w->starts.size() != p) w->starts.assign(p, 0);
    if (w->posts.size() != p) w->posts.assign(p, 0);
}
}  // namespace

// Exposure epoch: every origin of `group` may access this window until MPI_Win_wait
MSX_EXPORT int MPI_Win_post(MPI_Group group, int assert_, MPI_Win win)
{
    MSX_REQUIRE_INIT("MPI_Win_post");
    RmaWin* w;
    int rc = v_win(win, &w);
    if (rc != MPI_SUCCESS) return err_win(nullptr, "MPI_Win_post", rc);
    std::vector<int> origins;
    rc = group_window_ranks(w, group, &origins);
    if (rc == MPI_SUCCESS && w->exposure_epoch) {
        set_error("MPI_Win_post inside an exposure epoch (**rmasync)");
        rc = MPI_ERR_RMA_SYNC;
    }
    (void)assert_;                    // MPI_MODE_NOCHECK / NOSTORE / NOPUT: hints here
    if (rc == MPI_SUCCESS) {
        pscw_sizes(w);
        w->exposure_origins = origins;
        w->exposure_epoch = true;
        rc = engine_rma_post(w);
    }
    return err_win(w, "MPI_Win_post", rc);
}

// Access epoch: operations to `group`'s members are queued until
// MPI_Win_complete, which waits for their posts (MPID_Win_start only records
// the group, win.cpp:3775-3801)
MSX_EXPORT int MPI_Win_start(MPI_Group group, int assert_, MPI_Win win)
{
    MSX_REQUIRE_INIT("MPI_Win_start");
    RmaWin* w;
    int rc = v_win(win, &w);
    if (rc != MPI_SUCCESS) return err_win(nullptr, "MPI_Win_start", rc);
    std::vector<int> targets;
    rc = group_window_ranks(w, group, &targets);
    if (rc == MPI_SUCCESS && w->access_epoch) {
        set_error("MPI_Win_start inside an access epoch (**rmasync)");
        rc = MPI_ERR_RMA_SYNC;
    }
    if (rc == MPI_SUCCESS) {
        pscw_sizes(w);
        w->access_targets = targets;
        w->access_assert = assert_;
        w->access_epoch = true;
    }
    return err_win(w, "MPI_Win_start", rc);
}

// Every operation of the access epoch is applied at its target before the
// target's MPI_Win_wait can return.  Without a matching MPI_Win_start the
// reference dereferences a null group; here it is MPI_ERR_RMA_SYNC.
MSX_EXPORT int MPI_Win_complete(MPI_Win win)
{
    MSX_REQUIRE_INIT("MPI_Win_complete");
    RmaWin* w;
    int rc = v_win(win, &w);
    if (rc != MPI_SUCCESS) return err_win(nullptr, "MPI_Win_complete", rc);
    if (!w->access_epoch) {
        set_error("MPI_Win_complete without MPI_Win_start (**rmasync)");
        return err_win(w, "MPI_Win_complete", MPI_ERR_RMA_SYNC);
    }
    rc = engine_rma_complete(w);
    w->access_epoch = false;
    w->access_targets.clear();
    return err_win(w, "MPI_Win_complete", rc);
}

// MPID_Win_wait (win.cpp:4077-4088): returns once every origin of the posted
// group completed; with no exposure epoch open there is nothing to wait for
MSX_EXPORT int MPI_Win_wait(MPI_Win win)
{
    MSX_REQUIRE_INIT("MPI_Win_wait");
    RmaWin* w;
    int rc = v_win(win, &w);
    if (rc != MPI_SUCCESS) return err_win(nullptr, "MPI_Win_wait", rc);
    if (!w->exposure_epoch) return MPI_SUCCESS;
    int flag = 0;
    rc = engine_rma_wait(w, true, &flag);
    if (rc == MPI_SUCCESS) {
        w->exposure_epoch = false;
        w->exposure_origins.clear();
    }
    return err_win(w, "MPI_Win_wait", rc);
}

// MPID_Win_test (win.cpp:2001-2012): the non-blocking MPI_Win_wait
MSX_EXPORT int MPI_Win_test(MPI_Win win, int* flag)
{
    MSX_REQUIRE_INIT("MPI_Win_test");
    RmaWin* w;
    int rc = v_win(win, &w);
    if (rc != MPI_SUCCESS) return err_win(nullptr, "MPI_Win_test", rc);
    if (!flag) { set_error("null flag"); return err_win(w, "MPI_Win_test", MPI_ERR_ARG); }
    if (!w->exposure_epoch) { *flag = 1; return MPI_SUCCESS; }
    rc = engine_rma_wait(w, false, flag);
    if (rc == MPI_SUCCESS && *flag) {
        w->exposure_epoch = false;
        w->exposure_origins.clear();
    }
    return err_win(w, "MPI_Win_test", rc);
}

// api/mpi_win.cpp:979-1030: the group of the window's communicator
MSX_EXPORT int MPI_Win_get_group(MPI_Win win, MPI_Group* group)
{
    MSX_REQUIRE_INIT("MPI_Win_get_group");
    RmaWin* w;
    int rc = v_win(win, &w);
    if (rc != MPI_SUCCESS) return err_win(nullptr, "MPI_Win_get_group", rc);
    if (!group) { set_error("null group"); return err_win(w, "MPI_Win_get_group", MPI_ERR_ARG); }
    return err_win(w, "MPI_Win_get_group", group_create(w->comm->lpid, group));
}

// MPID_Win_lock_all: a shared lock on every rank (mpid/win.cpp:4133-4150)
MSX_EXPORT int MPI_Win_lock_all(int assert_, MPI_Win win)
{
    MSX_REQUIRE_INIT("MPI_Win_lock_all");
    RmaWin* w;
    int rc = v_win(win, &w);
    if (rc != MPI_SUCCESS) return err_win(nullptr, "MPI_Win_lock_all", rc);
    for (int r = 0; rc == MPI_SUCCESS && r < w->comm->size; ++r) rc = win_lock(w, MPI_LOCK_SHARED, r, assert_);
    if (rc == MPI_SUCCESS) w->lock_all = true;
    return err_win(w, "MPI_Win_lock_all", rc);
}

MSX_EXPORT int MPI_Win_unlock_all(MPI_Win win)
{
    MSX_REQUIRE_INIT("MPI_Win_unlock_all");
    RmaWin* w;
    int rc = v_win(win, &w);
    if (rc != MPI_SUCCESS) return err_win(nullptr, "MPI_Win_unlock_all", rc);
    if (!w->lock_all) {
        set_error("MPI_Win_unlock_all without MPI_Win_lock_all (**rmasync)");
        return err_win(w, "MPI_Win_unlock_all", MPI_ERR_OTHER);
    }
    for (int r = 0; r < w->comm->size; ++r) {
        const int r2 = w->lock_mode[(size_t)r] ? win_unlock(w, r) : MPI_SUCCESS;
        if (rc == MPI_SUCCESS) rc = r2;
    }
    w->lock_all = false;
    return err_win(w, "MPI_Win_unlock_all", rc);
}

// Flush: every operation this rank issued to `rank` is complete at origin and
// target (a fetch has landed; an update is visible to the target's next
// access).  flush_local needs only origin completion, which is the same here.
namespace {
int win_flush(const char* fn, int rank, MPI_Win win)
{
    MSX_REQUIRE_INIT(fn);
    RmaWin* w;
    int rc = v_win(win, &w);             // on failure w is null: the error goes to MPI_COMM_WORLD's handler
    if (rc == MPI_SUCCESS) rc = v_lock_rank(w, rank);
    if (rc == MPI_SUCCESS && rank != MPI_PROC_NULL) rc = engine_rma_flush(w, rank);
    return err_win(w, fn, rc);
}

int win_flush_all(const char* fn, MPI_Win win)
{
    MSX_REQUIRE_INIT(fn);
    RmaWin* w;
    int rc = v_win(win, &w);
    if (rc != MPI_SUCCESS) return err_win(nullptr, fn, rc);
    for (int r = 0; r < w->comm->size; ++r) {
        const int r2 = engine_rma_flush(w, r);
        if (rc == MPI_SUCCESS) rc = r2;
    }
    return err_win(w, fn, rc);
}
}  // namespace

MSX_EXPORT int MPI_Win_flush(int rank, MPI_Win win)
{
    return win_flush("MPI_Win_flush", rank, win);
}

MSX_EXPORT int MPI_Win_flush_local(int rank, MPI_Win win)
{
    return win_flush("MPI_Win_flush_local", rank, win);
}

MSX_EXPORT int MPI_Win_flush_all(MPI_Win win)
{
    return win_flush_all("MPI_Win_flush_all", win);
}

MSX_EXPORT int MPI_Win_flush_local_all(MPI_Win win)
{
    return win_flush_all("MPI_Win_flush_local_all", win);
}

// MPI_Win_sync: public and private copies of the window agree.  Remote
// updates are applied by this rank's own service thread on this GPU and are
// complete (stream-synchronised) before their origin's flush returns, so
// a memory fence for the host-side view is all that is left.
MSX_EXPORT int MPI_Win_sync(MPI_Win win)
{
    MSX_REQUIRE_INIT("MPI_Win_sync");
    RmaWin* w;
    int rc = v_win(win, &w);
    if (rc != MPI_SUCCESS) return err_win(nullptr, "MPI_Win_sync", rc);
    std::atomic_thread_fence(std::memory_order_seq_cst);
    return MPI_SUCCESS;
}

MSX_EXPORT int MPI_Win_set_errhandler(MPI_Win win, MPI_Errhandler eh)
{
    MSX_REQUIRE_INIT("MPI_Win_set_errhandler");
    RmaWin* w;
    int rc = v_win(win, &w);
    if (rc == MPI_SUCCESS && eh != MPI_ERRORS_ARE_FATAL && eh != MPI_ERRORS_RETURN) {
        set_error("unsupported errhandler 0x%x", eh);
        rc = MPI_ERR_ARG;
    }
    if (rc != MPI_SUCCESS) return err_win(w, "MPI_Win_set_errhandler", rc);
    w->errhandler = eh;
    return MPI_SUCCESS;
}

MSX_EXPORT int MPI_Win_get_errhandler(MPI_Win win, MPI_Errhandler* eh)
{
    MSX_REQUIRE_INIT("MPI_Win_get_errhandler");
    RmaWin* w;
    int rc = v_win(win, &w);
    if (rc == MPI_SUCCESS && !eh) rc = MPI_ERR_ARG;
    if (rc != MPI_SUCCESS) return err_win(w, "MPI_Win_get_errhandler", rc);
    *eh = w->errhandler == MPI_ERRHANDLER_NULL ? MPI_ERRORS_ARE_FATAL : w->errhandler;
    return MPI_SUCCESS;
}

// ---- data movement, plain and request-based (api/mpi_rma.cpp:187 MPI_Rput, 486 MPI_Rget,
// 813 MPI_Raccumulate, 1215 MPI_Rget_accumulate; MPID_Win_R* mpid/win.cpp:1324-1900).
// A request-based operation is validated and queued exactly as its plain form:
// one body each, rform = false for the plain call (request unused).  Its request
// must complete without a synchronisation call, so the target's queue is
// flushed at once (the reference completes the request when its queued
// operation has gone out, at the latest at the next flush / unlock) and a
// complete request is returned.  Passive-target epochs only (MPI-3 11.3.5):
// in a fence or PSCW epoch the call fails with MPI_ERR_RMA_SYNC.
namespace {
int rma_request_pre(RmaWin* w, MPI_Request* request, int target)
{
    if (!request) { set_error("**nullptr request"); return MPI_ERR_ARG; }
    *request = MPI_REQUEST_NULL;
    if (target != MPI_PROC_NULL && target >= 0 && target < w->comm->size && !w->lock_all &&
        !w->lock_mode[(size_t)target]) {
        set_error("request-based RMA outside a passive-target epoch on rank %d (**rmasync)", target);
        return MPI_ERR_RMA_SYNC;
    }
    return MPI_SUCCESS;
}

int rma_request_post(RmaWin* w, int target, int rc, MPI_Request* request)
{
    if (rc == MPI_SUCCESS && target != MPI_PROC_NULL) rc = engine_rma_flush(w, target);
    if (rc == MPI_SUCCESS) rc = request_completed_rma(request, MPI_SUCCESS);
    return rc;
}

int rma_put(const char* fn, const void* origin_addr, int origin_count, MPI_Datatype origin_datatype, int target_rank,
            MPI_Aint target_disp, int target_count, MPI_Datatype target_datatype, MPI_Win win, bool rform,
            MPI_Request* request)
{
    MSX_REQUIRE_INIT(fn);
    RmaWin* w;
    int rc = v_win(win, &w);             // on failure w is null: the error goes to MPI_COMM_WORLD's handler
    if (rc == MPI_SUCCESS && rform) rc = rma_request_pre(w, request, target_rank);
    if (rc == MPI_SUCCESS) rc = v_dtype_any(origin_addr, origin_count, origin_datatype);
    if (rc == MPI_SUCCESS) rc = v_target(w, target_count, target_datatype, target_rank, target_disp);
    if (rc == MPI_SUCCESS && target_rank != MPI_PROC_NULL && origin_count > 0)
        rc = v_match(origin_count, origin_datatype, target_count, target_datatype);
    if (rc == MPI_SUCCESS && target_rank != MPI_PROC_NULL && origin_count > 0)
        rc = rma_issue(w, RMA_PUT, target_rank, target_disp, O_REPLACE, origin_addr, origin_count, origin_datatype,
                       nullptr, 0, MPI_DATATYPE_NULL, target_count, target_datatype, nullptr);
    if (rc == MPI_SUCCESS && rform) rc = rma_request_post(w, target_rank, rc, request);
    return err_win(w, fn, rc);
}

int rma_get(const char* fn, void* origin_addr, int origin_count, MPI_Datatype origin_datatype, int target_rank,
            MPI_Aint target_disp, int target_count, MPI_Datatype target_datatype, MPI_Win win, bool rform,
            MPI_Request* request)
{
    MSX_REQUIRE_INIT(fn);
    RmaWin* w;
    int rc = v_win(win, &w);             // on failure w is null: the error goes to MPI_COMM_WORLD's handler
    if (rc == MPI_SUCCESS && rform) rc = rma_request_pre(w, request, target_rank);
    if (rc == MPI_SUCCESS) rc = v_dtype_any(origin_addr, origin_count, origin_datatype);
    if (rc == MPI_SUCCESS) rc = v_target(w, target_count, target_datatype, target_rank, target_disp);
    if (rc == MPI_SUCCESS && target_rank != MPI_PROC_NULL && origin_count > 0)
        rc = v_match(origin_count, origin_datatype, target_count, target_datatype);
    if (rc == MPI_SUCCESS && target_rank != MPI_PROC_NULL && origin_count > 0)
        rc = rma_issue(w, RMA_GET, target_rank, target_disp, O_NOOP, nullptr, 0, MPI_DATATYPE_NULL, origin_addr,
                       origin_count, origin_datatype, target_count, target_datatype, nullptr);
    if (rc == MPI_SUCCESS && rform) rc = rma_request_post(w, target_rank, rc, request);
    return err_win(w, fn, rc);
}

int rma_accumulate(const char* fn, const void* origin_addr, int origin_count, MPI_Datatype origin_datatype,
                   int target_rank, MPI_Aint target_disp, int target_count, MPI_Datatype target_datatype, MPI_Op op,
                   MPI_Win win, bool rform, MPI_Request* request)
{
    MSX_REQUIRE_INIT(fn);
    RmaWin* w;
    OpRef r;
    int rc = v_win(win, &w);             // on failure w is null: the error goes to MPI_COMM_WORLD's handler
    if (rc == MPI_SUCCESS && rform) rc = rma_request_pre(w, request, target_rank);
    if (rc == MPI_SUCCESS) rc = v_dtype_any(origin_addr, origin_count, origin_datatype);
    if (rc == MPI_SUCCESS) rc = rma_op(op, &r, false);        // MPI_NO_OP: **noopnotallowed
    if (rc == MPI_SUCCESS) rc = v_target(w, target_count, target_datatype, target_rank, target_disp);
    if (rc == MPI_SUCCESS && target_rank != MPI_PROC_NULL && origin_count > 0)
        rc = v_match(origin_count, origin_datatype, target_count, target_datatype);
    if (rc == MPI_SUCCESS && target_rank != MPI_PROC_NULL && origin_count > 0)
        rc = rma_issue(w, RMA_ACC, target_rank, target_disp, r.opidx, origin_addr, origin_count, origin_datatype,
                       nullptr, 0, MPI_DATATYPE_NULL, target_count, target_datatype, nullptr);
    if (rc == MPI_SUCCESS && rform) rc = rma_request_post(w, target_rank, rc, request);
    return err_win(w, fn, rc);
}

int rma_get_accumulate(const char* fn, const void* origin_addr, int origin_count, MPI_Datatype origin_datatype,
                       void* result_addr, int result_count, MPI_Datatype result_datatype, int target_rank,
                       MPI_Aint target_disp, int target_count, MPI_Datatype target_datatype, MPI_Op op, MPI_Win win,
                       bool rform, MPI_Request* request)
{
    MSX_REQUIRE_INIT(fn);
    RmaWin* w;
    OpRef r;
    int rc = v_win(win, &w);             // on failure w is null: the error goes to MPI_COMM_WORLD's handler
    if (rc == MPI_SUCCESS && rform) rc = rma_request_pre(w, request, target_rank);
    if (rc == MPI_SUCCESS) rc = v_op_handle(op, &r);
    const bool noop = rc == MPI_SUCCESS && r.opidx == O_NOOP;
    if (rc == MPI_SUCCESS && !noop) rc = v_dtype_any(origin_addr, origin_count, origin_datatype);
    if (rc == MPI_SUCCESS) rc = v_dtype_any(result_addr, result_count, result_datatype);
    if (rc == MPI_SUCCESS) rc = v_target(w, target_count, target_datatype, target_rank, target_disp);
    if (rc == MPI_SUCCESS) rc = rma_op(op, &r, true);
    if (rc == MPI_SUCCESS && target_rank != MPI_PROC_NULL && result_count > 0) {
        rc = v_match(result_count, result_datatype, target_count, target_datatype);
        if (rc == MPI_SUCCESS && !noop) rc = v_match(origin_count, origin_datatype, target_count, target_datatype);
    }
    if (rc == MPI_SUCCESS && target_rank != MPI_PROC_NULL && target_count > 0)
        rc = rma_issue(w, noop ? RMA_GET : RMA_GACC, target_rank, target_disp, r.opidx, origin_addr, origin_count,
                       origin_datatype, result_addr, result_count, result_datatype, target_count, target_datatype,
                       nullptr);
    if (rc == MPI_SUCCESS && rform) rc = rma_request_post(w, target_rank, rc, request);
    return err_win(w, fn, rc);
}
}  // namespace

MSX_EXPORT int MPI_Put(const void* origin_addr, int origin_count, MPI_Datatype origin_datatype, int target_rank,
                       MPI_Aint target_disp, int target_count, MPI_Datatype target_datatype, MPI_Win win)
{
    return rma_put("MPI_Put", origin_addr, origin_count, origin_datatype, target_rank, target_disp, target_count,
                   target_datatype, win, false, nullptr);
}

MSX_EXPORT int MPI_Get(void* origin_addr, int origin_count, MPI_Datatype origin_datatype, int target_rank,
                       MPI_Aint target_disp, int target_count, MPI_Datatype target_datatype, MPI_Win win)
{
    return rma_get("MPI_Get", origin_addr, origin_count, origin_datatype, target_rank, target_disp, target_count,
                   target_datatype, win, false, nullptr);
}

MSX_EXPORT int MPI_Accumulate(const void* origin_addr, int origin_count, MPI_Datatype origin_datatype,
                              int target_rank, MPI_Aint target_disp, int target_count,
                              MPI_Datatype target_datatype, MPI_Op op, MPI_Win win)
{
    return rma_accumulate("MPI_Accumulate", origin_addr, origin_count, origin_datatype, target_rank, target_disp,
                          target_count, target_datatype, op, win, false, nullptr);
}

MSX_EXPORT int MPI_Get_accumulate(const void* origin_addr, int origin_count, MPI_Datatype origin_datatype,
                                  void* result_addr, int result_count, MPI_Datatype result_datatype,
                                  int target_rank, MPI_Aint target_disp, int target_count,
                                  MPI_Datatype target_datatype, MPI_Op op, MPI_Win win)
{
    return rma_get_accumulate("MPI_Get_accumulate", origin_addr, origin_count, origin_datatype, result_addr,
                              result_count, result_datatype, target_rank, target_disp, target_count, target_datatype,
                              op, win, false, nullptr);
}

MSX_EXPORT int MPI_Rput(const void* origin_addr, int origin_count, MPI_Datatype origin_datatype, int target_rank,
                        MPI_Aint target_disp, int target_count, MPI_Datatype target_datatype, MPI_Win win,
                        MPI_Request* request)
{
    return rma_put("MPI_Rput", origin_addr, origin_count, origin_datatype, target_rank, target_disp, target_count,
                   target_datatype, win, true, request);
}

MSX_EXPORT int MPI_Rget(void* origin_addr, int origin_count, MPI_Datatype origin_datatype, int target_rank,
                        MPI_Aint target_disp, int target_count, MPI_Datatype target_datatype, MPI_Win win,
                        MPI_Request* request)
{
    return rma_get("MPI_Rget", origin_addr, origin_count, origin_datatype, target_rank, target_disp, target_count,
                   target_datatype, win, true, request);
}

MSX_EXPORT int MPI_Raccumulate(const void* origin_addr, int origin_count, MPI_Datatype origin_datatype,
                               int target_rank, MPI_Aint target_disp, int target_count,
                               MPI_Datatype target_datatype, MPI_Op op, MPI_Win win, MPI_Request* request)
{
    return rma_accumulate("MPI_Raccumulate", origin_addr, origin_count, origin_datatype, target_rank, target_disp,
                          target_count, target_datatype, op, win, true, request);
}

MSX_EXPORT int MPI_Rget_accumulate(const void* origin_addr, int origin_count, MPI_Datatype origin_datatype,
                                   void* result_addr, int result_count, MPI_Datatype result_datatype,
                                   int target_rank, MPI_Aint target_disp, int target_count,
                                   MPI_Datatype target_datatype, MPI_Op op, MPI_Win win, MPI_Request* request)
{
    return rma_get_accumulate("MPI_Rget_accumulate", origin_addr, origin_count, origin_datatype, result_addr,
                              result_count, result_datatype, target_rank, target_disp, target_count, target_datatype,
                              op, win, true, request);
}

MSX_EXPORT int MPI_Fetch_and_op(const void* origin_addr, void* result_addr, MPI_Datatype datatype,
                                int target_rank, MPI_Aint target_disp, MPI_Op op, MPI_Win win)
{
    MSX_REQUIRE_INIT("MPI_Fetch_and_op");
    RmaWin* w;
    int rc = v_win(win, &w);
    if (rc != MPI_SUCCESS) return err_win(nullptr, "MPI_Fetch_and_op", rc);
    OpRef r;
    rc = v_op_handle(op, &r);
    const bool noop = rc == MPI_SUCCESS && r.opidx == O_NOOP;
    if (rc == MPI_SUCCESS && !noop) rc = v_dtype(origin_addr, 1, datatype);
    if (rc == MPI_SUCCESS) rc = v_dtype(result_addr, 1, datatype);
    if (rc == MPI_SUCCESS) rc = v_target(w, 1, datatype, target_rank, target_disp);
    if (rc == MPI_SUCCESS) rc = rma_op(op, &r, true);
    if (rc == MPI_SUCCESS && target_rank != MPI_PROC_NULL)
        rc = rma_issue(w, noop ? RMA_GET : RMA_GACC, target_rank, target_disp, r.opidx, origin_addr, 1, datatype,
                       result_addr, 1, datatype, 1, datatype, nullptr);
    return err_win(w, "MPI_Fetch_and_op", rc);
}

MSX_EXPORT int MPI_Compare_and_swap(const void* origin_addr, const void* compare_addr, void* result_addr,
                                    MPI_Datatype datatype, int target_rank, MPI_Aint target_disp, MPI_Win win)
{
    MSX_REQUIRE_INIT("MPI_Compare_and_swap");
    RmaWin* w;
    int rc = v_win(win, &w);
    if (rc != MPI_SUCCESS) return err_win(nullptr, "MPI_Compare_and_swap", rc);
    rc = v_dtype(origin_addr, 1, datatype);
    if (rc == MPI_SUCCESS) rc = v_dtype(compare_addr, 1, datatype);
    if (rc == MPI_SUCCESS) rc = v_dtype(result_addr, 1, datatype);
    if (rc == MPI_SUCCESS) rc = v_target(w, 1, datatype, target_rank, target_disp);
    if (rc == MPI_SUCCESS && target_rank != MPI_PROC_NULL)
        rc = rma_issue(w, RMA_CAS, target_rank, target_disp, O_REPLACE, origin_addr, 1, datatype, result_addr, 1,
                       datatype, 1, datatype, compare_addr);
    return err_win(w, "MPI_Compare_and_swap", rc);
}

// ---- PMPI_ profiling aliases (dll/msmpi.def) --------------------------------
MSX_ALIAS(MPI_Win_post) int PMPI_Win_post(MPI_Group, int, MPI_Win);
MSX_ALIAS(MPI_Win_start) int PMPI_Win_start(MPI_Group, int, MPI_Win);
MSX_ALIAS(MPI_Win_complete) int PMPI_Win_complete(MPI_Win);
MSX_ALIAS(MPI_Win_wait) int PMPI_Win_wait(MPI_Win);
MSX_ALIAS(MPI_Win_test) int PMPI_Win_test(MPI_Win, int*);
MSX_ALIAS(MPI_Win_get_group) int PMPI_Win_get_group(MPI_Win, MPI_Group*);
MSX_ALIAS(MPI_Rput) int PMPI_Rput(const void*, int, MPI_Datatype, int, MPI_Aint, int, MPI_Datatype, MPI_Win,
                                  MPI_Request*);
MSX_ALIAS(MPI_Rget) int PMPI_Rget(void*, int, MPI_Datatype, int, MPI_Aint, int, MPI_Datatype, MPI_Win, MPI_Request*);
MSX_ALIAS(MPI_Raccumulate) int PMPI_Raccumulate(const void*, int, MPI_Datatype, int, MPI_Aint, int, MPI_Datatype,
                                                MPI_Op, MPI_Win, MPI_Request*);
MSX_ALIAS(MPI_Rget_accumulate) int PMPI_Rget_accumulate(const void*, int, MPI_Datatype, void*, int, MPI_Datatype, int,
                                                        MPI_Aint, int, MPI_Datatype, MPI_Op, MPI_Win, MPI_Request*);
MSX_ALIAS(MPI_Accumulate) int PMPI_Accumulate(const void*, int, MPI_Datatype, int, MPI_Aint, int, MPI_Datatype,
                                              MPI_Op, MPI_Win);
MSX_ALIAS(MPI_Get_accumulate) int PMPI_Get_accumulate(const void*, int, MPI_Datatype, void*, int, MPI_Datatype, int,
                                                      MPI_Aint, int, MPI_Datatype, MPI_Op, MPI_Win);
MSX_ALIAS(MPI_Fetch_and_op) int PMPI_Fetch_and_op(const void*, void*, MPI_Datatype, int, MPI_Aint, MPI_Op, MPI_Win);
