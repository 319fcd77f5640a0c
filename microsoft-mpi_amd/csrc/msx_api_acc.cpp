// msx_api_acc.cpp — the entry points of the typed accumulate family
// (include/msx.h): msx_accumulate_dev, msx_accumulate_widen_dev,
// msx_accumulate_batch_dev and msx_get_accumulate_dev, each with its plan entry.
//
// One static plan function stands behind each plan entry and its real call:
// msx.h's argument checks in their order, then the plan of msx_dtype_acc.cpp; it
// never touches a GPU.  The shared checks are stated once: v_committed_type
// (msx_dtype_api.cpp), v_builtin_op (msx_api.cpp) and the plans' own rules.
#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "msx_api.h"
#include "msx_dtype_acc.h"

using namespace msx;

// ---- msx_accumulate_dev: a combine between two datatype layouts ----------------
// Checks 1 - 6 of msx.h in their order (counts, v_committed_type, v_builtin_op,
// then dt_acc2_plan's) and, when they pass, the plan.
static int accumulate_plan(int64_t ocount, MPI_Datatype odt, int64_t tcount, MPI_Datatype tdt, MPI_Op op, OpRef* r,
                           Dtype** ot, Dtype** tt, Acc2Plan* plan)
{
    if (ocount < 0 || tcount < 0) { set_error("negative count"); return MPI_ERR_COUNT; }
    if (const int rc = v_committed_type(odt, ot)) return rc;
    if (const int rc = v_committed_type(tdt, tt)) return rc;
    if (const int rc = v_builtin_op(op, "msx_accumulate_dev", "one combine per element: use MPI_SUM", r)) return rc;
    return dt_acc2_plan(r->opidx, *ot, ocount, *tt, tcount, plan);
}

MSX_EXPORT int msx_accumulate_plan(int64_t origin_count, MPI_Datatype origin_type, int64_t target_count,
                                   MPI_Datatype target_type, MPI_Op op, int64_t* elements, int* path, int* granule)
{
    if (!elements || !path || !granule) { set_error("null plan output"); return MPI_ERR_ARG; }
    *elements = 0;
    *path = *granule = 0;
    OpRef r;
    Dtype *ot, *tt;
    Acc2Plan plan;
    const int rc = accumulate_plan(origin_count, origin_type, target_count, target_type, op, &r, &ot, &tt, &plan);
    if (rc != MPI_SUCCESS) return rc;
    *elements = plan.elements;
    *path = plan.path;
    *granule = plan.path ? plan.granule : 0;
    return MPI_SUCCESS;
}

MSX_EXPORT int msx_accumulate_dev(const void* origin, int64_t origin_count, MPI_Datatype origin_type, void* target,
                                  int64_t target_count, MPI_Datatype target_type, MPI_Op op, void* stream)
{
    OpRef r;
    Dtype *ot, *tt;
    Acc2Plan plan;
    int rc = accumulate_plan(origin_count, origin_type, target_count, target_type, op, &r, &ot, &tt, &plan);
    if (rc != MPI_SUCCESS || plan.path == 0) return rc;
    if (!origin || !target) { set_error("null buffer"); return MPI_ERR_BUFFER; }
    rc = ensure_device();
    if (rc != MPI_SUCCESS) return rc;
    return dt_acc2_dev(r.opidx, ot, origin_count, origin, tt, target, plan, static_cast<hipStream_t>(stream));
}

// ---- msx_accumulate_widen_dev: 16-bit float origins into fp32 targets -----------
// Checks 1 - 6 of msx.h in their order (msx_accumulate_dev's, then the ops this
// call has kernels for, then dt_accw2_plan's) and, when they pass, the plan.
static int accumulate_widen_plan(int64_t ocount, MPI_Datatype odt, int64_t tcount, MPI_Datatype tdt, MPI_Op op,
                                 OpRef* r, Dtype** ot, Dtype** tt, AccW2Plan* plan)
{
    if (ocount < 0 || tcount < 0) { set_error("negative count"); return MPI_ERR_COUNT; }
    if (const int rc = v_committed_type(odt, ot)) return rc;
    if (const int rc = v_committed_type(tdt, tt)) return rc;
    if (const int rc = v_builtin_op(op, "msx_accumulate_widen_dev", "the target is the fp32 accumulator: use MPI_SUM", r))
        return rc;
    switch (r->opidx) {
    case O_SUM: case O_PROD: case O_MAX: case O_MIN: case O_REPLACE: case O_NOOP: break;
    default:
        set_error("msx_accumulate_widen_dev takes MPI_SUM, MPI_PROD, MPI_MAX, MPI_MIN, MPI_REPLACE and MPI_NO_OP, not %s",
                  op_name(r->opidx));
        return MPI_ERR_OP;
    }
    return dt_accw2_plan(r->opidx, *ot, ocount, *tt, tcount, plan);
}

MSX_EXPORT int msx_accumulate_widen_plan(int64_t origin_count, MPI_Datatype origin_type, int64_t target_count,
                                         MPI_Datatype target_type, MPI_Op op, int64_t* elements, int* path)
{
    if (!elements || !path) { set_error("null plan output"); return MPI_ERR_ARG; }
    *elements = 0;
    *path = 0;
    OpRef r;
    Dtype *ot, *tt;
    AccW2Plan plan;
    const int rc = accumulate_widen_plan(origin_count, origin_type, target_count, target_type, op, &r, &ot, &tt, &plan);
    if (rc != MPI_SUCCESS) return rc;
    *elements = plan.elements;
    *path = plan.path;
    return MPI_SUCCESS;
}

MSX_EXPORT int msx_accumulate_widen_dev(const void* origin, int64_t origin_count, MPI_Datatype origin_type,
                                        void* target, int64_t target_count, MPI_Datatype target_type, MPI_Op op,
                                        void* stream)
{
    OpRef r;
    Dtype *ot, *tt;
    AccW2Plan plan;
    int rc = accumulate_widen_plan(origin_count, origin_type, target_count, target_type, op, &r, &ot, &tt, &plan);
    if (rc != MPI_SUCCESS || plan.path == 0) return rc;
    if (!origin || !target) { set_error("null buffer"); return MPI_ERR_BUFFER; }
    rc = ensure_device();
    if (rc != MPI_SUCCESS) return rc;
    return dt_accw2_dev(r.opidx, ot, origin, tt, target, plan, static_cast<hipStream_t>(stream));
}

// ---- msx_accumulate_batch_dev: many typed combines in few launches ---------------
// Checks 2 - 7 of msx.h in their order (2 for the four arrays a plan takes;
// v_committed_type per segment under a "segment i: " prefix, v_builtin_op, then
// dt_acc2_batch_plan's) and, when they pass, the plan.
static int accumulate_batch_plan(const int64_t* ocount, const MPI_Datatype* odt, const int64_t* tcount,
                                 const MPI_Datatype* tdt, int nseg, MPI_Op op, OpRef* r, Acc2BatchPlan* plan)
{
    if (nseg < 0 || !ocount || !odt || !tcount || !tdt) { set_error("bad segment arrays (nseg=%d)", nseg); return MPI_ERR_ARG; }
    for (int i = 0; i < nseg; ++i)
        if (ocount[i] < 0 || tcount[i] < 0) { set_error("negative count in segment %d", i); return MPI_ERR_COUNT; }
    std::vector<const Dtype*> ot((size_t)nseg), tt((size_t)nseg);
    for (int i = 0; i < nseg; ++i) {
        const MPI_Datatype dts[2] = {odt[i], tdt[i]};
        const Dtype** out[2] = {&ot[(size_t)i], &tt[(size_t)i]};
        for (int j = 0; j < 2; ++j) {
            Dtype* t = nullptr;
            const int rc = v_committed_type(dts[j], &t);
            if (rc != MPI_SUCCESS) {
                const std::string why = last_error();
                set_error("segment %d: %s", i, why.c_str());
                return rc;
            }
            *out[j] = t;
        }
    }
    if (const int rc = v_builtin_op(op, "msx_accumulate_batch_dev", "one combine per element: use MPI_SUM", r)) return rc;
    return dt_acc2_batch_plan(r->opidx, ot.data(), ocount, tt.data(), tcount, nseg, plan);
}

MSX_EXPORT int msx_accumulate_batch_plan(const int64_t* origin_count, const MPI_Datatype* origin_type,
                                         const int64_t* target_count, const MPI_Datatype* target_type, int nseg,
                                         MPI_Op op, int* width, int64_t* fuse_below, int* launches, int* batched,
                                         int* single)
{
    if (!width || !fuse_below || !launches || !batched || !single) { set_error("null plan output"); return MPI_ERR_ARG; }
    *width = acc2_batch_width();
    *fuse_below = acc2_batch_fuse_below();
    *launches = *batched = *single = 0;
    if (nseg == 0) return MPI_SUCCESS;
    OpRef r;
    Acc2BatchPlan plan;
    const int rc = accumulate_batch_plan(origin_count, origin_type, target_count, target_type, nseg, op, &r, &plan);
    if (rc != MPI_SUCCESS) return rc;
    *launches = plan.launches();
    *batched = plan.fused;
    *single = plan.single;
    return MPI_SUCCESS;
}

MSX_EXPORT int msx_accumulate_batch_dev(const void* const* origin, const int64_t* origin_count,
                                        const MPI_Datatype* origin_type, void* const* target,
                                        const int64_t* target_count, const MPI_Datatype* target_type, int nseg,
                                        MPI_Op op, void* stream)
{
    if (nseg == 0) return MPI_SUCCESS;
    if (!origin || !target) { set_error("bad segment arrays (nseg=%d)", nseg); return MPI_ERR_ARG; }
    OpRef r;
    Acc2BatchPlan plan;
    int rc = accumulate_batch_plan(origin_count, origin_type, target_count, target_type, nseg, op, &r, &plan);
    if (rc != MPI_SUCCESS || plan.steps.empty()) return rc;
    for (const Acc2BatchStep& st : plan.steps)
        if (!origin[st.seg] || !target[st.seg]) { set_error("null buffer in segment %d", st.seg); return MPI_ERR_BUFFER; }
    // two segments with one target address and one target datatype handle map
    // the same first element: they certainly collide (spans are not compared:
    // disjoint maps may interleave)
    std::vector<const Acc2BatchStep*> by_target;
    for (const Acc2BatchStep& st : plan.steps) by_target.push_back(&st);
    auto key = [&](const Acc2BatchStep* st) { return std::make_pair((uintptr_t)target[st->seg], target_type[st->seg]); };
    std::sort(by_target.begin(), by_target.end(), [&](const Acc2BatchStep* a, const Acc2BatchStep* b) {
        return key(a) != key(b) ? key(a) < key(b) : a->seg < b->seg;
    });
    for (size_t j = 1; j < by_target.size(); ++j)
        if (key(by_target[j]) == key(by_target[j - 1])) {
            set_error("target of segment %d is the target of segment %d (same address, same datatype)",
                      by_target[j]->seg, by_target[j - 1]->seg);
            return MPI_ERR_BUFFER;
        }
    rc = ensure_device();
    if (rc != MPI_SUCCESS) return rc;
    return dt_acc2_batch_dev(r.opidx, plan, origin, target, static_cast<hipStream_t>(stream));
}

// ---- msx_get_accumulate_dev: fetch and combine between three datatype layouts ----
// Checks 1 - 6 of msx.h in their order (counts, v_committed_type, v_builtin_op,
// then dt_gacc3_plan's) and, when they pass, the plan.
// *ot stays null under MPI_NO_OP: the origin triple is ignored there.
static int get_accumulate_plan(int64_t ocount, MPI_Datatype odt, int64_t rcount, MPI_Datatype rdt, int64_t tcount,
                               MPI_Datatype tdt, MPI_Op op, OpRef* r, Dtype** ot, Dtype** rt, Dtype** tt,
                               Acc3Plan* plan)
{
    const bool noop = op == MPI_NO_OP;
    if ((!noop && ocount < 0) || rcount < 0 || tcount < 0) { set_error("negative count"); return MPI_ERR_COUNT; }
    const MPI_Datatype dts[3] = {odt, rdt, tdt};
    Dtype** out[3] = {ot, rt, tt};
    *ot = nullptr;
    for (int i = noop ? 1 : 0; i < 3; ++i)
        if (const int rc = v_committed_type(dts[i], out[i])) return rc;
    if (const int rc = v_builtin_op(op, "msx_get_accumulate_dev", "one combine per element: use MPI_SUM", r)) return rc;
    return dt_gacc3_plan(r->opidx, *ot, ocount, *rt, rcount, *tt, tcount, plan);
}

MSX_EXPORT int msx_get_accumulate_plan(int64_t origin_count, MPI_Datatype origin_type, int64_t result_count,
                                       MPI_Datatype result_type, int64_t target_count, MPI_Datatype target_type,
                                       MPI_Op op, int64_t* elements, int* path, int* granule)
{
    if (!elements || !path || !granule) { set_error("null plan output"); return MPI_ERR_ARG; }
    *elements = 0;
    *path = *granule = 0;
    OpRef r;
    Dtype *ot, *rt, *tt;
    Acc3Plan plan;
    const int rc = get_accumulate_plan(origin_count, origin_type, result_count, result_type, target_count,
                                       target_type, op, &r, &ot, &rt, &tt, &plan);
    if (rc != MPI_SUCCESS) return rc;
    *elements = plan.elements;
    *path = plan.path;
    *granule = plan.path ? plan.granule : 0;
    return MPI_SUCCESS;
}

MSX_EXPORT int msx_get_accumulate_dev(const void* origin, int64_t origin_count, MPI_Datatype origin_type,
                                      void* result, int64_t result_count, MPI_Datatype result_type, void* target,
                                      int64_t target_count, MPI_Datatype target_type, MPI_Op op, void* stream)
{
    OpRef r;
    Dtype *ot, *rt, *tt;
    Acc3Plan plan;
    int rc = get_accumulate_plan(origin_count, origin_type, result_count, result_type, target_count, target_type, op,
                                 &r, &ot, &rt, &tt, &plan);
    if (rc != MPI_SUCCESS || plan.path == 0) return rc;
    if (!result || !target || (!origin && r.opidx != O_NOOP)) { set_error("null buffer"); return MPI_ERR_BUFFER; }
    rc = ensure_device();
    if (rc != MPI_SUCCESS) return rc;
    return dt_gacc3_dev(r.opidx, ot, origin, rt, result_count, result, tt, target, plan,
                        static_cast<hipStream_t>(stream));
}
