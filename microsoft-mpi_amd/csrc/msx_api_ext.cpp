// msx_api_ext.cpp — the msx_* extension and test-hook ABI (include/msx.h): build
// provenance, the builtin op table and op_errno, the device entry points, the
// kernel hooks, the tuning hooks and schedule introspection.
#include <algorithm>
#include <vector>

#include "msx_api.h"
#include "msx_dtype.h"
#include "msx_kernels.h"
#include "msx_transport.h"

using namespace msx;

// Build provenance: MSX_SOURCE_HASH is the SHA-256 prefix of the library's
// sources and headers at build time (Makefile), so a test can tell whether a
// prebuilt .so was compiled from the tree it ships with (tests/test_abi.py).
#ifndef MSX_SOURCE_HASH
#define MSX_SOURCE_HASH "unknown"
#endif
MSX_EXPORT const char* msx_version(void) { return "msmpi-mi355x 0.1 (gfx950) src=" MSX_SOURCE_HASH; }

MSX_EXPORT const char* msx_engine_transport(void)
{
    Comm* c = world();
    return engine_transport_name(c ? c->tp : nullptr);
}
MSX_EXPORT int msx_engine_gpu_shared(void)
{
    Comm* c = world();
    if (!c) return -1;
    return c->tp && c->tp->gpu_shared ? 1 : 0;
}
MSX_EXPORT int msx_engine_stats(double* out, int n, int reset)
{
    if (!out || n < 0) return -1;
    return engine_stats(out, n, reset);
}
MSX_EXPORT int msx_peer_write_bandwidth(int64_t bytes_per_peer, int reps, double* seconds, int64_t* bytes_used)
{
    MSX_REQUIRE_INIT("msx_peer_write_bandwidth");
    if (!seconds || !bytes_used || bytes_per_peer <= 0 || reps <= 0) return MPI_ERR_ARG;
    Comm* c = world();
    return engine_peer_write_probe(c, (size_t)bytes_per_peer, reps, seconds, bytes_used);
}
MSX_EXPORT int msx_device_count(void) { return device_count_noinit(); }
MSX_EXPORT const char* msx_last_error(void) { return last_error(); }

MSX_EXPORT int msx_op_check(MPI_Op op, MPI_Datatype dt)
{
    OpRef r;
    return v_op(op, dt, &r);
}

MSX_EXPORT int msx_type_size(MPI_Datatype dt) { return type_size(dt); }

// ---- the builtin op table (MPIR_Op_table, mpid/op.cpp:618-622, :703-1923) ----
// Each entry has the MPI_User_function shape the reference's internal callers
// bind to: NBC reduce tasks (mpid/tasks.cpp:667,680), RMA accumulate
// (mpid/win.cpp:1435, packethandling.cpp:2938,3046), the Fortran proxy
// (fortran/mpif.cpp:963-976) and MPID_Uop_call (include/op.h:171-174).  Like
// MPIR_Op_<op> they validate nothing up front: `*len` <= 0 does nothing (the
// reference loops `while(--len >= 0)`), and a datatype outside the op's table
// leaves inout untouched and sets the calling thread's op_errno to MPI_ERR_OP
// (op.cpp:732,...,1791; Mpi.CallState->op_errno, include/MpiCallState.h:13).
// Device operands (or pinned / pageable host memory, offloaded like
// MPI_Reduce_local) are combined by the gfx950 kernels; the call returns with
// the result in `inout`.  A failure of the GPU path also lands in op_errno.
namespace {
thread_local int t_op_errno = 0;

void op_entry(int opidx, void* in, void* inout, int* len, MPI_Datatype* dt)
{
    if (!len || !dt || *len <= 0) return;
    if (op_check_dtype(opidx, *dt) != MPI_SUCCESS) {
        set_error("**opundefined: builtin op %d on datatype 0x%x", opidx, *dt);
        t_op_errno = MPI_ERR_OP;
        return;
    }
    const int rc = reduce_local_any(opidx, type_info(*dt)->kind, in, inout, (size_t)*len);
    if (rc != MPI_SUCCESS) t_op_errno = rc;
}
}  // namespace

#define MSX_OP_ENTRY(fn, idx) \
    MSX_EXPORT void fn(void* in, void* inout, int* len, MPI_Datatype* dt) { op_entry(idx, in, inout, len, dt); }
MSX_OP_ENTRY(msx_op_max, O_MAX)
MSX_OP_ENTRY(msx_op_min, O_MIN)
MSX_OP_ENTRY(msx_op_sum, O_SUM)
MSX_OP_ENTRY(msx_op_prod, O_PROD)
MSX_OP_ENTRY(msx_op_land, O_LAND)
MSX_OP_ENTRY(msx_op_band, O_BAND)
MSX_OP_ENTRY(msx_op_lor, O_LOR)
MSX_OP_ENTRY(msx_op_bor, O_BOR)
MSX_OP_ENTRY(msx_op_lxor, O_LXOR)
MSX_OP_ENTRY(msx_op_bxor, O_BXOR)
MSX_OP_ENTRY(msx_op_minloc, O_MINLOC)
MSX_OP_ENTRY(msx_op_maxloc, O_MAXLOC)
#undef MSX_OP_ENTRY

// MPIR_Op_replace (op.cpp:1886-1903): MPIR_Localcopy(in -> inout), any datatype
MSX_EXPORT void msx_op_replace(void* in, void* inout, int* len, MPI_Datatype* dt)
{
    if (!len || !dt || *len <= 0) return;
    const int rc = local_copy(in, inout, (size_t)*len, *dt);
    if (rc != MPI_SUCCESS) t_op_errno = rc;
}

// MPIR_Op_noop (op.cpp:1906-1923)
MSX_EXPORT void msx_op_noop(void*, void*, int*, MPI_Datatype*) {}

// MPIR_Op_table[op % 16 - 1]: the entry of a builtin op handle
// (MPI_MAX .. MPI_NO_OP, 0x58000001 .. 0x5800000e), NULL for anything else --
// MSX_SUM_WIDE (0x58000050) included: op % 16 - 1 cannot name it, and a
// pairwise entry could not keep fp32 partials between calls.
MSX_EXPORT MPI_User_function* msx_op_table(MPI_Op op)
{
    static MPI_User_function* const kTable[] = {
        msx_op_max, msx_op_min, msx_op_sum, msx_op_prod, msx_op_land, msx_op_band, msx_op_lor,
        msx_op_bor, msx_op_lxor, msx_op_bxor, msx_op_minloc, msx_op_maxloc, msx_op_replace, msx_op_noop};
    static_assert(sizeof(kTable) / sizeof(kTable[0]) == O_NOOP, "one entry per builtin op");
    const int idx = op & 0xff;
    if ((op & ~0xff) != (MPI_MAX & ~0xff) || idx < O_MAX || idx > O_NOOP) return nullptr;
    return kTable[idx - 1];
}

// The routing test of the table binding: both operands in
// device memory.  Host operands stay on the reference's own MPIR_Op_<op> loop,
// which the offload beats only above ~1 MiB (bench.py host_path.crossover);
// the library itself has no CPU combine.  No GPU -> 0, without initialising one.
MSX_EXPORT int msx_operands_on_device(const void* in, const void* inout)
{
    if (!in || !inout || device_count_noinit() <= 0) return 0;
    return classify(in).place == Place::Device && classify(inout).place == Place::Device ? 1 : 0;
}

// Mpi.CallState->op_errno of the calling thread: read it, and clear it before
// a sequence of calls (the collectives do `op_errno = 0`, reduce.cpp:97,3794).
MSX_EXPORT int msx_op_errno(void) { return t_op_errno; }
MSX_EXPORT void msx_op_errno_reset(void) { t_op_errno = 0; }

MSX_EXPORT int msx_reduce_local_dev(const void* in, void* inout, int64_t count, MPI_Datatype dt,
                                    MPI_Op op, void* stream)
{
    if (count == 0) return MPI_SUCCESS;
    OpRef r;
    int rc = v_op(op, dt, &r);
    if (rc != MPI_SUCCESS) return rc;
    if (r.opidx == O_NULL && !r.dev_fn) {
        set_error("device entry point takes builtin ops and device user ops only");
        return MPI_ERR_OP;
    }
    if (count < 0) { set_error("negative count"); return MPI_ERR_COUNT; }
    if (!in || !inout) { set_error("null buffer"); return MPI_ERR_BUFFER; }
    if (in == inout) { set_error("inbuf aliases inoutbuf"); return MPI_ERR_BUFFER; }
    rc = ensure_device();
    if (rc != MPI_SUCCESS) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);   // NULL = the HIP null stream
    // a device user op: its own launch on the caller's stream, enqueue only
    if (r.dev_fn) return device_op_call(r, dt, in, inout, (size_t)count, s);
    return reduce_local_device(r.opidx, type_info(dt)->kind, in, inout, (size_t)count, s);
}

// ---- msx_fetch_and_op_dev: the combine that hands back the old inout ----------
// msx_reduce_local_dev's checks in its order with `fetched` added (msx.h);
// MPI_REPLACE and MPI_NO_OP are legal here as in MPI_Fetch_and_op, on any
// predefined datatype.
MSX_EXPORT int msx_fetch_and_op_dev(const void* in, void* fetched, void* inout, int64_t count, MPI_Datatype dt,
                                    MPI_Op op, void* stream)
{
    if (count == 0) return MPI_SUCCESS;
    OpRef r;
    int rc = v_op_handle(op, &r);
    if (rc != MPI_SUCCESS) return rc;
    if (r.opidx == O_NULL) { set_error("msx_fetch_and_op_dev takes builtin ops only"); return MPI_ERR_OP; }
    const bool moves_bytes = r.opidx == O_REPLACE || r.opidx == O_NOOP;
    int esz;
    if (moves_bytes) {
        esz = type_size(dt);       // a pair type's whole struct, padding included
        if (esz <= 0) {
            set_error("MPI_Op 0x%x (%s) takes a predefined datatype with data, not 0x%x", op, op_name(r.opidx), dt);
            return MPI_ERR_OP;
        }
    } else {
        rc = op_check_dtype(r.opidx, dt);
        if (rc != MPI_SUCCESS || !type_info(dt)) {
            set_error("MPI_Op 0x%x (%s) is not defined for datatype 0x%x", op, op_name(r.opidx), dt);
            return MPI_ERR_OP;
        }
        esz = type_info(dt)->size;
    }
    if (count < 0 || (uint64_t)count > (UINT64_MAX >> 2) / (uint64_t)esz) {
        set_error("bad count (%lld)", (long long)count);
        return MPI_ERR_COUNT;
    }
    const bool noop = r.opidx == O_NOOP;
    if (!inout || !fetched || (!in && !noop)) { set_error("null buffer"); return MPI_ERR_BUFFER; }
    if (!noop && in == inout) { set_error("inbuf aliases inoutbuf"); return MPI_ERR_BUFFER; }
    const size_t nb = (size_t)count * (size_t)esz;
    const uintptr_t f = (uintptr_t)fetched, io = (uintptr_t)inout, a = (uintptr_t)in;
    if (f < io + nb && io < f + nb) { set_error("fetched overlaps inout"); return MPI_ERR_BUFFER; }
    if (!noop && f < a + nb && a < f + nb) { set_error("fetched overlaps in"); return MPI_ERR_BUFFER; }
    rc = ensure_device();
    if (rc != MPI_SUCCESS) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);   // NULL = the HIP null stream
    hipError_t e;
    if (noop) {
        const void* ps = inout;
        void* pd = fetched;
        e = launch_copy_segs(&ps, &pd, &nb, 1, s);
    } else if (r.opidx == O_REPLACE) {
        e = launch_fetch_combine(O_REPLACE, K_U8, in, fetched, inout, nb, s);
    } else {
        e = launch_fetch_combine(r.opidx, type_info(dt)->kind, in, fetched, inout, (size_t)count, s);
    }
    return e == hipSuccess ? MPI_SUCCESS : hip_fail(e, "fetch-and-combine kernel launch");
}

// ---- msx_reduce_local_batch_dev: many small combines in few launches ---------
namespace {
// Mutually misaligned segments (operands at different offsets from 16-byte
// alignment) run element by element inside a fused launch below this many
// bytes per operand and take their own launch_combine (k_combine_shift) from
// it on.
constexpr size_t kBatchScalarMax = (size_t)64 << 10;

// What one batch call does with its non-empty segments, in index order: a
// fused segment joins the open fused launch, which is issued when it holds
// kCombineSegsWidth segments and at the end; a single one is launched on its
// own where it stands.
struct BatchStep {
    int seg;
    bool fused;
};
struct BatchPlan {
    std::vector<BatchStep> steps;
    int fused = 0, single = 0;
    int launches() const { return (fused + kCombineSegsWidth - 1) / kCombineSegsWidth + single; }
};

struct ByteRange {
    uintptr_t lo, hi;
    int seg;
};

// Checks 2-6 of msx_reduce_local_batch_dev (msx.h) and, when they pass, the
// plan.  One function behind the plan entry and the real call.
int batch_plan(const void* const* in, void* const* inout, const int64_t* counts, int nseg, MPI_Datatype dt, MPI_Op op,
               OpRef* r, BatchPlan* plan)
{
    if (nseg < 0 || !in || !inout || !counts) { set_error("bad segment arrays (nseg=%d)", nseg); return MPI_ERR_ARG; }
    int rc = v_op(op, dt, r);
    if (rc != MPI_SUCCESS) return rc;
    if (r->opidx == O_NULL || !type_info(dt)) { set_error("batch entry point takes builtin ops only"); return MPI_ERR_OP; }
    const size_t es = (size_t)type_info(dt)->size;
    for (int i = 0; i < nseg; ++i)
        if (counts[i] < 0 || (uint64_t)counts[i] > (UINT64_MAX >> 1) / es) {
            set_error("bad count of segment %d (%lld)", i, (long long)counts[i]);
            return MPI_ERR_COUNT;
        }
    for (int i = 0; i < nseg; ++i)
        if (counts[i] > 0 && (!in[i] || !inout[i])) { set_error("null buffer in segment %d", i); return MPI_ERR_BUFFER; }
    std::vector<ByteRange> wr, rd;
    for (int i = 0; i < nseg; ++i) {
        if (counts[i] == 0) continue;
        if (in[i] == inout[i]) { set_error("inbuf aliases inoutbuf in segment %d", i); return MPI_ERR_BUFFER; }
        const size_t nb = (size_t)counts[i] * es;
        rd.push_back({(uintptr_t)in[i], (uintptr_t)in[i] + nb, i});
        wr.push_back({(uintptr_t)inout[i], (uintptr_t)inout[i] + nb, i});
    }
    // no inout range may meet another inout range or any in range: the inout
    // ranges sorted by start are disjoint when each starts at or after the end
    // of the one before; every in range is then looked up among them
    std::sort(wr.begin(), wr.end(), [](const ByteRange& a, const ByteRange& b) { return a.lo < b.lo; });
    for (size_t j = 1; j < wr.size(); ++j)
        if (wr[j].lo < wr[j - 1].hi) {
            set_error("inout of segment %d overlaps inout of segment %d", wr[j].seg, wr[j - 1].seg);
            return MPI_ERR_BUFFER;
        }
    for (const ByteRange& x : rd) {
        auto w = std::upper_bound(wr.begin(), wr.end(), x.lo, [](uintptr_t v, const ByteRange& b) { return v < b.hi; });
        if (w != wr.end() && w->lo < x.hi) {
            set_error("inout of segment %d overlaps in of segment %d", w->seg, x.seg);
            return MPI_ERR_BUFFER;
        }
    }
    for (int i = 0; i < nseg; ++i) {
        if (counts[i] == 0) continue;
        const size_t nb = (size_t)counts[i] * es;
        const bool apart = ((uintptr_t)in[i] & 15) != ((uintptr_t)inout[i] & 15);
        const bool fused = nb < kCombineSegsMaxBytes && !(apart && nb >= kBatchScalarMax);
        plan->steps.push_back({i, fused});
        ++(fused ? plan->fused : plan->single);
    }
    return MPI_SUCCESS;
}
}  // namespace

MSX_EXPORT int msx_reduce_local_batch_plan(const void* const* in, void* const* inout, const int64_t* counts, int nseg,
                                           MPI_Datatype dt, MPI_Op op, int* width, int* launches, int* batched,
                                           int* single)
{
    if (!width || !launches || !batched || !single) { set_error("null plan output"); return MPI_ERR_ARG; }
    *width = kCombineSegsWidth;
    *launches = *batched = *single = 0;
    if (nseg == 0) return MPI_SUCCESS;
    OpRef r;
    BatchPlan plan;
    const int rc = batch_plan(in, inout, counts, nseg, dt, op, &r, &plan);
    if (rc != MPI_SUCCESS) return rc;
    *launches = plan.launches();
    *batched = plan.fused;
    *single = plan.single;
    return MPI_SUCCESS;
}

MSX_EXPORT int msx_reduce_local_batch_dev(const void* const* in, void* const* inout, const int64_t* counts, int nseg,
                                          MPI_Datatype dt, MPI_Op op, void* stream)
{
    if (nseg == 0) return MPI_SUCCESS;
    OpRef r;
    BatchPlan plan;
    int rc = batch_plan(in, inout, counts, nseg, dt, op, &r, &plan);
    if (rc != MPI_SUCCESS) return rc;
    if (plan.steps.empty()) return MPI_SUCCESS;         // every segment empty
    rc = ensure_device();
    if (rc != MPI_SUCCESS) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);   // NULL = the HIP null stream
    const Kind k = type_info(dt)->kind;
    CombineSeg segs[kCombineSegsWidth];
    int n = 0, left = plan.fused;
    for (const BatchStep& st : plan.steps) {
        const int i = st.seg;
        if (!st.fused) {
            // large and far-misaligned segments: launch_combine's own kernels and geometry
            rc = reduce_local_device(r.opidx, k, in[i], inout[i], (size_t)counts[i], s);
            if (rc != MPI_SUCCESS) return rc;
            continue;
        }
        segs[n++] = CombineSeg{in[i], inout[i], (size_t)counts[i]};
        if (n == kCombineSegsWidth || n == left) {
            hipError_t e = launch_combine_segs(r.opidx, k, segs, n, s);
            if (e != hipSuccess) return hip_fail(e, "batch combine kernel launch");
            left -= n;
            n = 0;
        }
    }
    return MPI_SUCCESS;
}

// one MPI_Reduce_local-sized vector split over the node's GPUs
// (ngpus <= 0: all visible), host operands over each GPU's own PCIe link;
// MPI_Reduce_local's checks, error codes returned (no error handler).
MSX_EXPORT int msx_reduce_local_multi(const void* in, void* inout, int64_t count, MPI_Datatype dt, MPI_Op op,
                                      int ngpus)
{
    if (count == 0) return MPI_SUCCESS;
    OpRef r;
    int rc = v_op(op, dt, &r);
    if (rc != MPI_SUCCESS) return rc;
    if (r.opidx == O_NULL || !type_info(dt)) { set_error("multi-GPU entry point takes builtin ops only"); return MPI_ERR_OP; }
    if (count < 0) { set_error("negative count"); return MPI_ERR_COUNT; }
    if (!in || !inout) { set_error("null buffer"); return MPI_ERR_BUFFER; }
    if (in == inout) { set_error("inbuf aliases inoutbuf"); return MPI_ERR_BUFFER; }
    return reduce_local_multi(r.opidx, type_info(dt)->kind, in, inout, (size_t)count, ngpus);
}

MSX_EXPORT int msx_reduce_tree_dev(const void* const* srcs, int p, void* out, int64_t count,
                                   MPI_Datatype dt, MPI_Op op, void* stream)
{
    if (count == 0) return MPI_SUCCESS;
    OpRef r;
    int rc = v_op(op, dt, &r);
    if (rc != MPI_SUCCESS) return rc;
    if (r.opidx == O_NULL) { set_error("device entry point takes builtin ops only"); return MPI_ERR_OP; }
    if (count < 0) { set_error("negative count"); return MPI_ERR_COUNT; }
    if (!srcs || !out || !(p == 1 || p == 2 || p == 4 || p == 8 || p == 16)) {
        set_error("bad tree arguments (p=%d)", p);
        return MPI_ERR_ARG;
    }
    rc = ensure_device();
    if (rc != MPI_SUCCESS) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);   // NULL = the HIP null stream
    hipError_t e = launch_tree(r.opidx, type_info(dt)->kind, srcs, p, out, (size_t)count, s);
    return e == hipSuccess ? MPI_SUCCESS : hip_fail(e, "tree kernel launch");
}

namespace {
// The shape the tree hooks below take: P leaves, a power of two <= 16, nleaves
// <= P of them present, no pair bit past leaf P; or a chain over 1..16 sources
// (pairmask ignored).  strict: what a device op's tree function is promised -- a
// chain has >= 2 sources and no pairmask / nleaves, a tree no pair bit at or past its absent leaves.
bool tree_shape_ok(const void* const* srcs, const void* out, int P, unsigned pairmask, int nleaves, int chain,
                   bool strict)
{
    if (!srcs || !out) return false;
    const bool pow2 = P >= 1 && P <= 16 && (P & (P - 1)) == 0;
    if (chain)
        return strict ? (P >= 2 && P <= 16 && pairmask == 0 && nleaves == 0)
                      : (P >= 1 && P <= 16 && nleaves >= 0 && nleaves <= P);
    return pow2 && nleaves >= 0 && nleaves <= P && (pairmask >> (strict && nleaves ? nleaves : P)) == 0;
}

// sources, pairmask, nleaves and chain of a TreeSpec from a checked shape
TreeSpec tree_spec_of(const void* const* srcs, int P, unsigned pairmask, int nleaves, int chain)
{
    TreeSpec t;
    t.P = P;
    t.chain = chain != 0;
    t.pairmask = chain ? 0 : pairmask;
    t.nleaves = chain ? 0 : nleaves;
    const int ns = chain ? P : 2 * P;
    for (int i = 0; i < ns; ++i) t.src[i] = srcs[i];
    return t;
}
}  // namespace

// Any reference-order tree the engine evaluates (TreeSpec): P leaves (a power
// of two <= 16) over srcs[2k] (leaf k) and srcs[2k+1] (its fold pair when bit
// k of pairmask is set), leaves >= nleaves absent (0 = all present); or, with
// chain set, the left-deep chain over srcs[0..P-1].  Stream-ordered, device
// pointers.  For tests and probes of the tree kernels outside a collective.
MSX_EXPORT int msx_reduce_tree_spec_dev(const void* const* srcs, int P, unsigned pairmask, int nleaves, int chain,
                                        void* out, int64_t count, MPI_Datatype dt, MPI_Op op, void* stream)
{
    if (count == 0) return MPI_SUCCESS;
    OpRef r;
    int rc = v_op(op, dt, &r);
    if (rc != MPI_SUCCESS) return rc;
    if (r.opidx == O_NULL) { set_error("device entry point takes builtin ops only"); return MPI_ERR_OP; }
    if (count < 0) { set_error("negative count"); return MPI_ERR_COUNT; }
    if (!tree_shape_ok(srcs, out, P, pairmask, nleaves, chain, false)) {
        set_error("bad tree spec (P=%d pairmask=0x%x nleaves=%d chain=%d)", P, pairmask, nleaves, chain);
        return MPI_ERR_ARG;
    }
    rc = ensure_device();
    if (rc != MPI_SUCCESS) return rc;
    const TreeSpec t = tree_spec_of(srcs, P, pairmask, nleaves, chain);
    hipError_t e = launch_tree_spec(r.opidx, type_info(dt)->kind, t, out, (size_t)count, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? MPI_SUCCESS : hip_fail(e, "tree kernel launch");
}

// A device user op's tree function (msx_op_create_device_tree) on the caller's
// memory and stream: the call a collective makes, without the collective.
// Never the pairwise path: an op without a tree function is MPI_ERR_OP and a
// decline comes back as MSX_TREE_DECLINED.
MSX_EXPORT int msx_reduce_tree_user_dev(const void* const* srcs, int P, unsigned pairmask, int nleaves, int chain,
                                        int in_left, void* out, int64_t count, MPI_Datatype dt, MPI_Op op,
                                        void* stream)
{
    OpRef r;
    int rc = v_op_handle(op, &r);
    if (rc != MPI_SUCCESS) return rc;
    if (!r.dev_tree) { set_error("MPI_Op 0x%x has no device tree function", op); return MPI_ERR_OP; }
    if (!tree_shape_ok(srcs, out, P, pairmask, nleaves, chain, true) || (in_left != 0 && in_left != 1)) {
        set_error("bad tree spec (P=%d pairmask=0x%x nleaves=%d chain=%d in_left=%d)", P, pairmask, nleaves, chain,
                  in_left);
        return MPI_ERR_ARG;
    }
    if (count < 0) { set_error("negative count"); return MPI_ERR_COUNT; }
    if (count == 0) return MPI_SUCCESS;
    rc = ensure_device();
    if (rc != MPI_SUCCESS) return rc;      // no GPU: MPI_ERR_OTHER, the function is never entered
    return device_op_tree_call(r, dt, srcs, P, pairmask, nleaves, chain != 0, in_left, out, (size_t)count,
                               static_cast<hipStream_t>(stream));
}

// The engine's local copy (the collect step of the collectives, MPIR_Localcopy
// of device data, mpid/pt2pt.cpp:929-948): k_copy_segs' XCD-contiguous 4-KiB
// tiles up to 16 MiB, k_copy_dram's one-wave dispatch-order grid above.
// Stream-ordered, device pointers (tests of the copy kernels).
MSX_EXPORT int msx_copy_dev(void* dst, const void* src, int64_t bytes, void* stream)
{
    if (bytes < 0 || (bytes > 0 && (!dst || !src))) return MPI_ERR_ARG;
    if (bytes == 0) return MPI_SUCCESS;
    int rc = ensure_device();
    if (rc != MPI_SUCCESS) return rc;
    const void* ps = src;
    void* pd = dst;
    size_t n = (size_t)bytes;
    hipError_t e = launch_copy_segs(&ps, &pd, &n, 1, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? MPI_SUCCESS : hip_fail(e, "copy kernel launch");
}

// msx_reduce_tree_spec_dev plus the TreeSpec fields only a collective sets
// (extra destinations, the result-ready count and its flags), so the tree
// kernels' write-through stores and tree_done run outside a collective.  Every
// pointer is the caller's device memory; nothing is allocated or freed here.
MSX_EXPORT int msx_reduce_tree_done_dev(const void* const* srcs, int P, unsigned pairmask, int nleaves, int chain,
                                        void* out, void* const* extra, int nextra, unsigned* done_counter,
                                        int done_launches, unsigned long long* const* done_flags, int done_nflags,
                                        unsigned long long done_seq, int64_t count, MPI_Datatype dt, MPI_Op op,
                                        void* stream)
{
    OpRef r;
    int rc = v_op(op, dt, &r);
    if (rc != MPI_SUCCESS) return rc;
    if (r.opidx == O_NULL) { set_error("device entry point takes builtin ops only"); return MPI_ERR_OP; }
    if (count < 0 || !tree_shape_ok(srcs, out, P, pairmask, nleaves, chain, false)) {
        set_error("bad tree spec (P=%d pairmask=0x%x nleaves=%d chain=%d count=%lld)", P, pairmask, nleaves, chain,
                  (long long)count);
        return MPI_ERR_ARG;
    }
    if (nextra < 0 || nextra > 31 || (nextra > 0 && !extra)) {
        set_error("bad extra destinations (nextra=%d)", nextra);
        return MPI_ERR_ARG;
    }
    for (int e = 0; e < nextra; ++e)
        if (!extra[e]) { set_error("null extra destination %d", e); return MPI_ERR_ARG; }
    if (done_nflags < 0 || done_nflags > 64 || (done_nflags > 0 && (!done_flags || !done_counter)) ||
        (done_counter && done_launches < 1)) {
        set_error("bad result-ready count (nflags=%d launches=%d)", done_nflags, done_launches);
        return MPI_ERR_ARG;
    }
    for (int i = 0; i < done_nflags; ++i)
        if (!done_flags[i]) { set_error("null result-ready flag %d", i); return MPI_ERR_ARG; }
    if (count == 0) return MPI_SUCCESS;
    rc = ensure_device();
    if (rc != MPI_SUCCESS) return rc;
    TreeSpec t = tree_spec_of(srcs, P, pairmask, nleaves, chain);
    t.nextra = nextra;
    for (int e = 0; e < nextra; ++e) t.extra[e] = extra[e];
    if (done_counter) {
        t.done_counter = done_counter;
        t.done_launches = (unsigned)done_launches;
        t.done_nflags = done_nflags;
        for (int i = 0; i < done_nflags; ++i) t.done_flags[i] = done_flags[i];
        t.done_seq = done_seq;
    }
    hipError_t e = launch_tree_spec(r.opidx, type_info(dt)->kind, t, out, (size_t)count, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? MPI_SUCCESS : hip_fail(e, "tree kernel launch");
}

namespace {
// (src, dst, nbytes) triples of the two segment hooks: arrays present, sizes
// not negative, a pointer for every non-empty segment
int v_segs(const void* const* src, void* const* dst, const int64_t* nbytes, int nseg, std::vector<size_t>* nb)
{
    if (nseg > 0 && (!src || !dst || !nbytes)) { set_error("null segment array"); return MPI_ERR_ARG; }
    nb->resize((size_t)nseg);
    for (int i = 0; i < nseg; ++i) {
        if (nbytes[i] < 0 || (nbytes[i] > 0 && (!src[i] || !dst[i]))) {
            set_error("bad segment %d (%lld bytes)", i, (long long)nbytes[i]);
            return MPI_ERR_ARG;
        }
        (*nb)[(size_t)i] = (size_t)nbytes[i];
    }
    return MPI_SUCCESS;
}
}  // namespace

// The push of the GPU-flag schedules (k_push_wait) over the caller's segments,
// flags and counter block (kCountWords zeroed words, left zero).  The launch's
// waiting workgroup is given no flag to wait for (wait_n = 0): it only reads
// *wait_flags once and never writes *wait_err, which must both be device words.
MSX_EXPORT int msx_push_dev(const void* const* src, void* const* dst, const int64_t* nbytes, int nseg,
                            unsigned long long* const* flags, int nflags, unsigned long long seq, unsigned* counter,
                            const unsigned long long* wait_flags, int* wait_err, void* stream)
{
    if (nseg < 0 || nseg > 32) { set_error("push takes 0..32 segments (nseg=%d)", nseg); return MPI_ERR_ARG; }
    std::vector<size_t> nb;
    int rc = v_segs(src, dst, nbytes, nseg, &nb);
    if (rc != MPI_SUCCESS) return rc;
    if (nflags < 0 || nflags > 64 || (nflags > 0 && !flags) || (nseg > 0 && !counter) || !wait_flags || !wait_err) {
        set_error("bad push flags (nflags=%d)", nflags);
        return MPI_ERR_ARG;
    }
    for (int i = 0; i < nflags; ++i)
        if (!flags[i]) { set_error("null flag %d", i); return MPI_ERR_ARG; }
    rc = ensure_device();
    if (rc != MPI_SUCCESS) return rc;
    hipError_t e = launch_push_wait(src, dst, nb.data(), nseg, flags, nflags, seq, counter, wait_flags, 0, -1, wait_err,
                                    static_cast<hipStream_t>(stream));
    return e == hipSuccess ? MPI_SUCCESS : hip_fail(e, "push kernel launch");
}

// The engine's multi-segment copy (k_copy_segs, the collect of allgather
// blocks): any number of segments, batched by the launcher.
MSX_EXPORT int msx_copy_segs_dev(const void* const* src, void* const* dst, const int64_t* nbytes, int nseg,
                                 void* stream)
{
    if (nseg < 0) { set_error("negative segment count"); return MPI_ERR_ARG; }
    std::vector<size_t> nb;
    int rc = v_segs(src, dst, nbytes, nseg, &nb);
    if (rc != MPI_SUCCESS) return rc;
    if (nseg == 0) return MPI_SUCCESS;
    rc = ensure_device();
    if (rc != MPI_SUCCESS) return rc;
    hipError_t e = launch_copy_segs(src, dst, nb.data(), nseg, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? MPI_SUCCESS : hip_fail(e, "copy kernel launch");
}

// Test hook: the pack/unpack/accumulate kernel geometry (0 = by size, the
// default; 1 = grid-stride form; 2 = tile form at every size), so small test
// cases run the kernels the default takes at large sizes.
MSX_EXPORT int msx_tune_pack(int mode)
{
    return pack_tune_set(mode) == 0 ? MPI_SUCCESS : MPI_ERR_ARG;
}

MSX_EXPORT int msx_set_staging_chunk(int64_t bytes)
{
    if (bytes <= 0) return MPI_ERR_ARG;
    set_staging_chunk((size_t)bytes);
    return MPI_SUCCESS;
}

MSX_EXPORT int msx_set_host_mode(int mode)
{
    if (mode < 0 || mode > 2) { set_error("host mode must be 0, 1 or 2"); return MPI_ERR_ARG; }
    set_host_mode(mode);
    return MPI_SUCCESS;
}

// ---- schedule introspection (host-side tests of the collective engine) ------
// which: 0 = allreduce tree of newrank n, 1 = reduce_scatter (recursive
// halving) tree of newrank n, 2 = pairwise chain of real rank n.
// src32 receives real ranks per kernel slot (-1 = unused).
MSX_EXPORT int msx_schedule_tree(int which, int p, int n, int* src32, int* P, unsigned* pairmask,
                                 int* chain)
{
    if (p < 1 || !src32 || !P || !pairmask || !chain) return MPI_ERR_ARG;
    // the tree kernels take 16 leaves: the fold trees (16 leaves, each a rank
    // or a folded pair) reach p = 31, the binomial tree (a leaf per rank) and
    // the chain (a source per rank) p = 16
    const bool fold = which == 0 || which == 1 || which == 3;
    if (p > (fold ? 31 : 16) || n < 0 || n >= p) return MPI_ERR_ARG;
    RankTree t;
    if (which == 0) t = tree_allreduce(p, n);
    else if (which == 1) t = tree_reduce_scatter(p, n);
    else if (which == 2) t = tree_pairwise(p, n);
    else if (which == 3) t = tree_reduce_rsag(p, n);
    else if (which == 4) t = tree_reduce_binomial(p, n);
    else return MPI_ERR_ARG;
    for (int i = 0; i < 32; ++i) src32[i] = t.src[i];
    *P = t.P;
    if (t.nleaves) {   // absent leaves are reported as -1
        for (int i = 2 * t.nleaves; i < 32; ++i) src32[i] = -1;
    }
    *pairmask = t.pairmask;
    *chain = t.chain ? 1 : 0;
    return MPI_SUCCESS;
}

// The spec a device-op collective hands to the op's tree function
// (devop_tree_spec, msx_schedule.cpp): which 0 allreduce for real rank n,
// 1 reduce for root n, 2 reduce_scatter for real rank n.
MSX_EXPORT int msx_schedule_devop_tree(int which, int p, int n, int commutative, int64_t total_count, int type_size,
                                       int* src32, int* P, unsigned* pairmask, int* nleaves, int* chain, int* in_left)
{
    if (!src32 || !P || !pairmask || !nleaves || !chain || !in_left || which < 0 || which > 2 || p < 1 || n < 0 ||
        n >= p || total_count < 0 || type_size < 0)
        return MPI_ERR_ARG;
    RankTree t;
    int il = 0;
    if (!devop_tree_spec((UserColl)which, p, n, commutative != 0, (size_t)total_count, type_size, &t, &il))
        return MPI_ERR_ARG;
    const int used = t.chain ? t.P : 2 * (t.nleaves ? t.nleaves : t.P);
    for (int i = 0; i < 32; ++i) src32[i] = i < used ? t.src[i] : -1;
    *P = t.P;
    *pairmask = t.pairmask;
    *nleaves = t.nleaves;
    *chain = t.chain ? 1 : 0;
    *in_left = il;
    return MPI_SUCCESS;
}

// The combine plan both user-op paths execute (userop_plan, msx_schedule.cpp):
// which 0 allreduce, 2 reduce_scatter, 3 scan (exclusive: exscan) for real
// rank n, 1 reduce for root n.  steps[2k], steps[2k + 1] = in, io of step k.
// MPI_ERR_ARG with *nsteps set when the plan has more than cap steps.
MSX_EXPORT int msx_schedule_userop_plan(int which, int p, int n, int commutative, int exclusive, int64_t total_count,
                                        int type_size, int* steps, int cap, int* nsteps, int* result)
{
    if (!steps || !nsteps || !result || cap < 0 || which < 0 || which > 3 || p < 1 || n < 0 || n >= p ||
        total_count < 0 || type_size < 0)
        return MPI_ERR_ARG;
    const CombinePlan plan =
        userop_plan((UserColl)which, p, n, commutative != 0, exclusive != 0, (size_t)total_count, type_size);
    *nsteps = (int)plan.steps.size();
    *result = plan.result;
    if (*nsteps > cap) return MPI_ERR_ARG;
    for (int k = 0; k < *nsteps; ++k) {
        steps[2 * k] = plan.steps[(size_t)k].in;
        steps[2 * k + 1] = plan.steps[(size_t)k].io;
    }
    return MPI_SUCCESS;
}

// which: 0 = allreduce algorithm, 1 = reduce_scatter algorithm (Algo enum)
MSX_EXPORT int msx_schedule_algo(int which, int p, int64_t count, int type_size)
{
    if (which == 0) return allreduce_algo(p, (size_t)count, type_size, true);
    if (which == 2) return reduce_algo(p, (size_t)count, type_size, true);
    return reduce_scatter_algo(p, (size_t)count, type_size, true);
}

// The same, with the gate's bytes per element taken from the datatype as the
// reference does: MPI_Type_size for the blocking calls and every reduce_scatter,
// the extent for the NBC task lists of MPI_Iallreduce / MPI_Ireduce (nbc = 1).
MSX_EXPORT int msx_schedule_algo_dt(int which, int p, int64_t count, MPI_Datatype dt, int nbc)
{
    if (!dtype_lookup(dt)) return -1;
    const int gate = gate_type_size(dt, which != 1 && nbc != 0);
    return msx_schedule_algo(which, p, count, gate);
}

// MPI_Ireduce's Rabenseifner tree of newrank n for `root` (root-relative ranks,
// reduce.cpp:6267-6670); same reporting as msx_schedule_tree
MSX_EXPORT int msx_schedule_ireduce_tree(int p, int n, int root, int* src32, int* P, unsigned* pairmask,
                                         int* chain)
{
    if (p < 1 || p > 16 || root < 0 || root >= p || !src32 || !P || !pairmask || !chain) return MPI_ERR_ARG;
    const RankTree t = tree_ireduce_rsag(p, n, root);
    for (int i = 0; i < 32; ++i) src32[i] = t.src[i];
    *P = t.P;
    *pairmask = t.pairmask;
    *chain = 0;
    return MPI_SUCCESS;
}

// newrank of `rank`, and the allreduce block owned by newrank n
MSX_EXPORT int msx_schedule_newrank(int rank, int p) { return newrank_of(rank, p); }
// The Rabenseifner schedules' piece plan for one rank (tests; piece_plan, the
// function both schedules run) with chunks of chunk_el elements, the caller's
// choice: *chunk_el_out = chunk_el, and every range of that rank's pieces over
// all chunks as (first element, end element, owner newrank) triples in
// out[3i..]; returns the number of ranges, or -1 when `cap` triples do not
// suffice.
MSX_EXPORT int64_t msx_schedule_pieces(int p, int64_t count, int64_t chunk_el, int rank, int64_t* chunk_el_out,
                                       int64_t* out, int64_t cap)
{
    if (p < 2 || p > 32 || count <= 0 || chunk_el < 0 || rank < 0 || rank >= p || !chunk_el_out || !out) return -1;
    *chunk_el_out = chunk_el;
    if (chunk_el == 0) return 0;
    const size_t pc = (size_t)chunk_el;
    Pieces pieces;
    int64_t n = 0;
    for (size_t o = 0; o < (size_t)count; o += pc) {
        piece_plan(p, (size_t)count, o, std::min(pc, (size_t)count - o), rank, &pieces);
        for (const TwoStepRange& g : pieces.ranges) {
            if (n >= cap) return -1;
            out[3 * n] = (int64_t)(o + g.e0);
            out[3 * n + 1] = (int64_t)(o + g.e1);
            out[3 * n + 2] = g.owner;
            ++n;
        }
    }
    return n;
}

// The same with the pipelined two-step allreduce / reduce's own chunk length
// for elements of esz bytes (0: the window is too small, no ranges).
MSX_EXPORT int64_t msx_schedule_two_step(int p, int64_t count, int esz, int rank, int64_t* chunk_el, int64_t* out,
                                         int64_t cap)
{
    if (p < 2 || p > 32 || esz <= 0) return -1;
    return msx_schedule_pieces(p, count, (int64_t)two_step_chunk_el(p, (size_t)esz), rank, chunk_el, out, cap);
}

MSX_EXPORT int msx_schedule_block(int p, int64_t count, int n, int64_t* start, int64_t* len)
{
    size_t s, l;
    allreduce_block(p, (size_t)count, allreduce_block_of_newrank(p, n), &s, &l);
    *start = (int64_t)s;
    *len = (int64_t)l;
    return MPI_SUCCESS;
}
