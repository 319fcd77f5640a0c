// msx_dtype_acc.cpp — the typed accumulate family (see msx_dtype_acc.h): plans
// and launches of the combines between two and three datatype layouts.
// The rules the plans share are the helpers below, each stated once; device
// layouts and their alignment come from dev_sides (msx_dtype.cpp).
#include "msx_dtype_acc.h"

#include <algorithm>
#include <initializer_list>
#include <string>

#include "msx_comm.h"
#include "msx_kernels.h"
#include "msx_runtime.h"

namespace msx {

namespace {

// The first `bytes` (> 0) data bytes of the type's instances lie in one piece
// at *disp: inside the first run, or over one-run instances that touch.
bool contiguous_prefix(const Dtype* t, int64_t bytes, int64_t* disp)
{
    const DtRun first = t->rn ? DtRun{t->rfirst, t->rlen} : t->runs[0];
    DtRun r{0, 0};
    *disp = first.disp;
    return bytes <= first.len || (single_run(t, &r) && t->size == t->extent);
}

// One (type, count) pair of a call, by the name the messages give it.  A null
// type is a pair the call ignores (the origin under MPI_NO_OP).
struct Side {
    const Dtype* t;
    int64_t count;
    const char* name;
};

// No pair's data bytes pass 2^62, so the plans' byte counts cannot overflow.
int counts_fit(std::initializer_list<Side> sides)
{
    const int64_t lim = (int64_t)1 << 62;
    for (const Side& x : sides)
        if (x.t && x.t->size > 0 && x.count > lim / x.t->size) {
            set_error("count overflows the data size");
            return MPI_ERR_COUNT;
        }
    return MPI_SUCCESS;
}

// Basic elements of `count` instances of `t`, `bytes` data bytes.  n_elements
// also counts the MPI_LB / MPI_UB markers of a struct (a subarray has two).
int64_t element_count(const Dtype* t, int64_t count, int64_t bytes)
{
    return t->el_size > 0 ? bytes / t->el_size : count * t->n_elements;
}

// Every side has one basic element type (a mixed struct and the pair types
// have none).
int single_element_types(std::initializer_list<Side> sides)
{
    for (const Side& x : sides)
        if (x.t->eltype == MPI_DATATYPE_NULL) {
            set_error("%s datatype has no single basic element type", x.name);
            return MPI_ERR_TYPE;
        }
    return MPI_SUCCESS;
}

// The element-type rules of a builtin op's combine, the target last: one basic
// element type per side, every side of the target's kind, and the op defined
// for each.
int element_rules(int opidx, std::initializer_list<Side> sides)
{
    if (const int rc = single_element_types(sides)) return rc;
    const Dtype* tt = (sides.end() - 1)->t;
    const TypeInfo* ti = type_info(tt->eltype);
    for (const Side* x = sides.begin(); x != sides.end() - 1; ++x) {
        const TypeInfo* xi = type_info(x->t->eltype);
        if ((xi ? xi->kind : K_NONE) != (ti ? ti->kind : K_NONE)) {
            set_error("%s elements 0x%x and target elements 0x%x differ in kind", x->name, x->t->eltype, tt->eltype);
            return MPI_ERR_TYPE;
        }
    }
    for (const Side& x : sides)
        if (!type_info(x.t->eltype) || op_check_dtype(opidx, x.t->eltype) != MPI_SUCCESS) {
            set_error("%s is not defined for datatype 0x%x", op_name(opidx), x.t->eltype);
            return MPI_ERR_OP;
        }
    return MPI_SUCCESS;
}

// Neither type map of a two-sided call splits an element (osz / tsz bytes).
int elements_whole(const Dtype* ot, int64_t osz, const Dtype* tt, int64_t tsz)
{
    if (runs_hold_elements(ot, osz) && runs_hold_elements(tt, tsz)) return MPI_SUCCESS;
    set_error("datatype runs split elements of 0x%x", tt->eltype);
    return MPI_ERR_TYPE;
}

int launched(hipError_t e, const char* what) { return e == hipSuccess ? MPI_SUCCESS : hip_fail(e, what); }

}  // namespace

// Checks 4 - 6 of msx_accumulate_dev (msx.h), by the helpers above, and the call's path.
int dt_acc2_plan(int opidx, const Dtype* ot, int64_t ocount, const Dtype* tt, int64_t tcount, Acc2Plan* p)
{
    *p = Acc2Plan();
    const Side o{ot, ocount, "origin"}, t{tt, tcount, "target"};
    if (const int rc = counts_fit({o, t})) return rc;
    const int64_t obytes = ocount * ot->size, tbytes = tcount * tt->size;
    if (obytes > tbytes) {
        set_error("accumulate truncated: %lld origin bytes into %lld", (long long)obytes, (long long)tbytes);
        return MPI_ERR_TRUNCATE;
    }
    p->elements = element_count(ot, ocount, obytes);
    p->bytes = obytes;
    if (obytes == 0 || opidx == O_NOOP) return MPI_SUCCESS;
    if (opidx == O_REPLACE) {
        p->granule = std::min(layout_align(ot), layout_align(tt));
    } else {
        if (const int rc = element_rules(opidx, {o, t})) return rc;
        const int64_t tsz = type_info(tt->eltype)->size;
        if (const int rc = elements_whole(ot, type_info(ot->eltype)->size, tt, tsz)) return rc;
        p->granule = (int)tsz;
    }
    const bool oc = contiguous_prefix(ot, obytes, &p->od), tc = contiguous_prefix(tt, obytes, &p->td);
    if (oc && tc) p->path = 1;
    else if (oc && obytes % tt->size == 0) p->path = 2;      // dt_acc_dev covers whole target instances
    else if (tc && opidx == O_REPLACE) p->path = 3;
    else p->path = 4;
    return MPI_SUCCESS;
}

int dt_acc2_dev(int opidx, const Dtype* ot, int64_t ocount, const void* origin, const Dtype* tt, void* target,
                const Acc2Plan& p, hipStream_t s)
{
    if (p.path == 0) return MPI_SUCCESS;
    const char* src = static_cast<const char*>(origin) + p.od;    // paths 1, 2: the origin's one piece
    char* dst = static_cast<char*>(target) + p.td;                // paths 1, 3: the target's
    const TypeInfo* ti = type_info(tt->eltype);                   // an op's element (checked by the plan)
    switch (p.path) {
    case 1: {
        if (opidx != O_REPLACE) return reduce_local_device(opidx, ti->kind, src, dst, (size_t)(p.bytes / ti->size), s);
        const void* ps = src;
        void* pd = dst;
        const size_t nb = (size_t)p.bytes;
        return launched(launch_copy_segs(&ps, &pd, &nb, 1, s), "copy kernel launch");
    }
    case 2:
        return dt_acc_dev(opidx, tt, p.bytes / tt->size, src, target, s);
    case 3:
        return dt_pack_dev(ot, ocount, origin, dst, s);
    default:
        break;
    }
    DevSide sd[2] = {{ot, origin}, {tt, target}};
    if (const int rc = dev_sides(sd, 2)) return rc;
    const int align = std::min(sd[0].align, sd[1].align);
    return launched(opidx == O_REPLACE
                        ? launch_dt_copy2(*sd[0].L, origin, *sd[1].L, target, p.bytes, align, s)
                        : launch_dt_acc2(opidx, ti->kind, *sd[0].L, origin, *sd[1].L, target, p.bytes / ti->size,
                                         align, s),
                    "two-layout datatype accumulate");
}

// ---- msx_accumulate_widen_dev: 16-bit float origins into fp32 targets ------------
// Checks 4 - 6 of msx_accumulate_widen_dev (msx.h): the shared count bound and
// first element rule, its own two, and the call's path.
int dt_accw2_plan(int opidx, const Dtype* ot, int64_t ocount, const Dtype* tt, int64_t tcount, AccW2Plan* p)
{
    *p = AccW2Plan();
    const Side o{ot, ocount, "origin"}, t{tt, tcount, "target"};
    if (const int rc = counts_fit({o, t})) return rc;
    const int64_t obytes = ocount * ot->size, tbytes = tcount * tt->size;
    if (obytes > tbytes / 2) {      // 2 * obytes > tbytes
        set_error("widening accumulate truncated: %lld origin bytes (twice that widened) into %lld",
                  (long long)obytes, (long long)tbytes);
        return MPI_ERR_TRUNCATE;
    }
    p->elements = element_count(ot, ocount, obytes);
    p->bytes = obytes;
    if (obytes == 0 || opidx == O_NOOP) return MPI_SUCCESS;
    if (const int rc = single_element_types({o, t})) return rc;
    const TypeInfo* oi = type_info(ot->eltype);
    const TypeInfo* ti = type_info(tt->eltype);
    if (!oi || (oi->kind != K_F16 && oi->kind != K_BF16)) {
        set_error("origin elements 0x%x are neither MSX_FLOAT16 nor MSX_BFLOAT16", ot->eltype);
        return MPI_ERR_TYPE;
    }
    if (!ti || ti->kind != K_F32) {
        set_error("target elements 0x%x are not 4-byte floats", tt->eltype);
        return MPI_ERR_TYPE;
    }
    if (const int rc = elements_whole(ot, oi->size, tt, ti->size)) return rc;
    const bool oc = contiguous_prefix(ot, obytes, &p->od), tc = contiguous_prefix(tt, 2 * obytes, &p->td);
    p->path = oc && tc ? 1 : 2;
    return MPI_SUCCESS;
}

int dt_accw2_dev(int opidx, const Dtype* ot, const void* origin, const Dtype* tt, void* target, const AccW2Plan& p,
                 hipStream_t s)
{
    if (p.path == 0) return MPI_SUCCESS;
    const Kind k = type_info(ot->eltype)->kind;                    // checked by the plan
    const int64_t n = p.bytes / 2;
    if (p.path == 1)
        return launched(launch_widen_combine(opidx, k, static_cast<const char*>(origin) + p.od,
                                             static_cast<char*>(target) + p.td, (size_t)n, s),
                        "widening accumulate");
    DevSide sd[2] = {{ot, origin}, {tt, target}};
    if (const int rc = dev_sides(sd, 2)) return rc;
    const bool aligned = sd[0].align >= 2 && sd[1].align >= 4;
    return launched(launch_dt_accw2(opidx, k, *sd[0].L, origin, *sd[1].L, target, n, aligned, s),
                    "two-layout widening accumulate");
}

// ---- msx_accumulate_batch_dev: many typed combines in few launches --------------
int acc2_batch_width() { return kAcc2SegsWidth; }
int64_t acc2_batch_fuse_below() { return kAcc2SegsFuseBelow; }
int Acc2BatchPlan::launches() const { return (fused + kAcc2SegsWidth - 1) / kAcc2SegsWidth + single; }

// Checks 6 and 7 of msx_accumulate_batch_dev (msx.h) and what the call does with
// each non-empty segment: a pure function of the host-side types, the counts
// and the op.
int dt_acc2_batch_plan(int opidx, const Dtype* const* ot, const int64_t* ocount, const Dtype* const* tt,
                       const int64_t* tcount, int nseg, Acc2BatchPlan* plan)
{
    *plan = Acc2BatchPlan();
    for (int i = 0; i < nseg; ++i) {
        Acc2BatchStep st;
        const int rc = dt_acc2_plan(opidx, ot[i], ocount[i], tt[i], tcount[i], &st.plan);
        if (rc != MPI_SUCCESS) {
            const std::string why = last_error();
            set_error("segment %d: %s", i, why.c_str());
            return rc;
        }
        if (st.plan.path == 0) continue;      // no origin data bytes, or MPI_NO_OP
        st.seg = i;
        st.ot = ot[i];
        st.tt = tt[i];
        st.ocount = ocount[i];
        // The fused kernels divide in 32 bits.  The granule is at least one
        // byte (MPI_REPLACE's depends on the pointers, which a plan does not
        // see), so sizes in bytes bound the sizes in granules.
        st.fused = st.plan.bytes < kAcc2SegsFuseBelow && dt_map_narrow(st.plan.bytes, ot[i]->size, tt[i]->size);
        plan->steps.push_back(st);
    }
    if (opidx != O_REPLACE)
        for (const Acc2BatchStep& st : plan->steps) {
            const Acc2BatchStep& s0 = plan->steps[0];
            if (type_info(st.tt->eltype)->kind != type_info(s0.tt->eltype)->kind) {
                set_error("segment %d has elements 0x%x and segment %d elements 0x%x: one element kind per call",
                          s0.seg, s0.tt->eltype, st.seg, st.tt->eltype);
                return MPI_ERR_TYPE;
            }
        }
    for (const Acc2BatchStep& st : plan->steps) ++(st.fused ? plan->fused : plan->single);
    return MPI_SUCCESS;
}

int dt_acc2_batch_dev(int opidx, const Acc2BatchPlan& plan, const void* const* origin, void* const* target,
                      hipStream_t s)
{
    if (plan.steps.empty()) return MPI_SUCCESS;
    // every fused segment's device layout before the first launch (a single
    // segment builds its own in dt_acc2_dev), with dt_acc2_dev's alignment:
    // both layouts and both pointers
    std::vector<Acc2Seg> segs;
    segs.reserve((size_t)plan.fused);
    for (const Acc2BatchStep& st : plan.steps) {
        if (!st.fused) continue;
        DevSide sd[2] = {{st.ot, origin[st.seg]}, {st.tt, target[st.seg]}};
        if (const int rc = dev_sides(sd, 2)) return rc;
        segs.push_back(Acc2Seg{sd[0].L, origin[st.seg], sd[1].L, target[st.seg], st.plan.bytes,
                               std::min(sd[0].align, sd[1].align)});
    }
    const Kind k = opidx == O_REPLACE ? K_NONE : type_info(plan.steps[0].tt->eltype)->kind;
    size_t at = 0;      // segs[at, at + n): the fused segments met since the last fused launch
    int n = 0;
    for (const Acc2BatchStep& st : plan.steps) {
        if (!st.fused) {
            const int rc = dt_acc2_dev(opidx, st.ot, st.ocount, origin[st.seg], st.tt, target[st.seg], st.plan, s);
            if (rc != MPI_SUCCESS) return rc;
            continue;
        }
        if (++n == kAcc2SegsWidth || at + (size_t)n == segs.size()) {
            const hipError_t e = opidx == O_REPLACE ? launch_dt_copy2_segs(&segs[at], n, s)
                                                    : launch_dt_acc2_segs(opidx, k, &segs[at], n, s);
            if (e != hipSuccess) return hip_fail(e, "batched two-layout datatype accumulate");
            at += (size_t)n;
            n = 0;
        }
    }
    return MPI_SUCCESS;
}

// Checks 4 - 6 of msx_get_accumulate_dev (msx.h), by the helpers above, and the call's
// path.  `ot` is null under MPI_NO_OP, where the result triple counts the elements.
int dt_gacc3_plan(int opidx, const Dtype* ot, int64_t ocount, const Dtype* rt, int64_t rcount, const Dtype* tt,
                  int64_t tcount, Acc3Plan* p)
{
    *p = Acc3Plan();
    const Side o{ot, ocount, "origin"}, r{rt, rcount, "result"}, t{tt, tcount, "target"};
    if (const int rc = counts_fit({o, r, t})) return rc;
    const Side& n = ot ? o : r;                          // the triple that counts the elements
    const int64_t nbytes = n.count * n.t->size;
    const int64_t rbytes = rcount * rt->size, tbytes = tcount * tt->size;
    if (nbytes > tbytes) {
        set_error("accumulate truncated: %lld origin bytes into %lld", (long long)nbytes, (long long)tbytes);
        return MPI_ERR_TRUNCATE;
    }
    if (nbytes > rbytes) {
        set_error("get_accumulate truncated: %lld target bytes into %lld of the result", (long long)nbytes,
                  (long long)rbytes);
        return MPI_ERR_TRUNCATE;
    }
    p->elements = element_count(n.t, n.count, nbytes);
    p->bytes = nbytes;
    if (nbytes == 0) return MPI_SUCCESS;
    if (opidx == O_NOOP) {
        p->granule = std::min(layout_align(rt), layout_align(tt));
    } else if (opidx == O_REPLACE) {
        p->granule = std::min({layout_align(ot), layout_align(rt), layout_align(tt)});
    } else {
        if (const int rc = element_rules(opidx, {o, r, t})) return rc;
        const int64_t tsz = type_info(tt->eltype)->size;
        for (const Dtype* x : {ot, rt, tt})
            if (!runs_hold_elements(x, tsz)) {
                set_error("datatype runs split elements of 0x%x", x->eltype);
                return MPI_ERR_TYPE;
            }
        p->granule = (int)tsz;
    }
    const bool oc = !ot || contiguous_prefix(ot, nbytes, &p->od);
    const bool rc1 = contiguous_prefix(rt, nbytes, &p->rd), tc = contiguous_prefix(tt, nbytes, &p->td);
    p->path = oc && rc1 && tc ? 1 : (opidx == O_NOOP ? 2 : 3);
    return MPI_SUCCESS;
}

int dt_gacc3_dev(int opidx, const Dtype* ot, const void* origin, const Dtype* rt, int64_t rcount, void* result,
                 const Dtype* tt, void* target, const Acc3Plan& p, hipStream_t s)
{
    if (p.path == 0) return MPI_SUCCESS;
    if (p.path == 1) {
        char* res = static_cast<char*>(result) + p.rd;
        char* dst = static_cast<char*>(target) + p.td;
        hipError_t e;
        if (opidx == O_NOOP) {
            const void* ps = dst;
            void* pd = res;
            const size_t nb = (size_t)p.bytes;
            e = launch_copy_segs(&ps, &pd, &nb, 1, s);
        } else {
            const char* src = static_cast<const char*>(origin) + p.od;
            const TypeInfo* ti = type_info(tt->eltype);       // an op's element (checked by the plan)
            e = opidx == O_REPLACE ? launch_fetch_combine(opidx, K_U8, src, res, dst, (size_t)p.bytes, s)
                                   : launch_fetch_combine(opidx, ti->kind, src, res, dst, (size_t)(p.bytes / ti->size), s);
        }
        return launched(e, "fetch-and-combine kernel launch");
    }
    if (p.path == 2) {
        // MPI_NO_OP: the typed -> typed copy target -> result.  Over whole target
        // instances it is msx_accumulate_dev's plan; a prefix that ends inside
        // an instance is what only the two-layout kernel covers.
        Acc2Plan q;
        if (p.bytes % tt->size == 0) {
            const int rc = dt_acc2_plan(O_REPLACE, tt, p.bytes / tt->size, rt, rcount, &q);
            if (rc != MPI_SUCCESS) return rc;
        } else {
            q.bytes = p.bytes;
            q.path = 4;
        }
        return dt_acc2_dev(O_REPLACE, tt, p.bytes / tt->size, target, rt, result, q, s);
    }
    DevSide sd[3] = {{ot, origin}, {rt, result}, {tt, target}};
    if (const int rc = dev_sides(sd, 3)) return rc;
    const int align = std::min({sd[0].align, sd[1].align, sd[2].align});
    const TypeInfo* ti = type_info(tt->eltype);
    return launched(opidx == O_REPLACE
                        ? launch_dt_xchg3(*sd[0].L, origin, *sd[1].L, result, *sd[2].L, target, p.bytes, align, s)
                        : launch_dt_gacc3(opidx, ti->kind, *sd[0].L, origin, *sd[1].L, result, *sd[2].L, target,
                                          p.bytes / ti->size, align, s),
                    "three-layout datatype get-accumulate");
}

}  // namespace msx
