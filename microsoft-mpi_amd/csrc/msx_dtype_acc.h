// msx_dtype_acc.h — the typed accumulate family (msx.h: msx_accumulate_dev,
// msx_accumulate_widen_dev, msx_accumulate_batch_dev, msx_get_accumulate_dev):
// combines between two or three datatype layouts, neither side packed.  Each
// member is a plan (a pure function of the host-side types, the counts and the
// op) and a *_dev function that does what the plan says.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>

#include "msx_dtype.h"

namespace msx {

// msx_accumulate_dev (msx.h): target elem e = origin elem e (op) target elem e
// over TWO type maps, e below the origin's element count.  dt_acc2_plan runs the
// call's checks 4 - 6 on the host-side types (no GPU is touched) and says what
// the call does; dt_acc2_dev does exactly that: paths 1 - 3 forward to the
// contiguous combine / copy, dt_acc_dev / dt_unpack_dev and dt_pack_dev, path 4
// is the two-layout kernel of msx_acc2.hip.
struct Acc2Plan {
    int64_t elements = 0;   // basic elements of the origin
    int64_t bytes = 0;      // data bytes of the origin
    int path = 0;           // 0 nothing to do, 1 - 4 as in msx.h
    int granule = 0;        // bytes one work item moves (16-byte aligned bases)
    int64_t od = 0, td = 0; // where the origin's / target's one piece starts (paths 1 - 3)
};
int dt_acc2_plan(int opidx, const Dtype* origin_t, int64_t origin_count, const Dtype* target_t,
                 int64_t target_count, Acc2Plan* plan);
int dt_acc2_dev(int opidx, const Dtype* origin_t, int64_t origin_count, const void* origin,
                const Dtype* target_t, void* target, const Acc2Plan& plan, hipStream_t s);

// msx_accumulate_widen_dev (msx.h): target elem e = F_op(target elem e,
// W(origin elem e)) over two type maps, the origin's elements MSX_FLOAT16 or
// MSX_BFLOAT16 and the target's fp32.  dt_accw2_plan runs the call's checks
// 4 - 6 on the host-side types (no GPU is touched; the shared rules are the
// ones dt_acc2_plan uses) and says what the call does;
// dt_accw2_dev does exactly that: path 1 is the streaming kernel of
// msx_widen.hip on the two pieces, path 2 its two-layout kernel.
struct AccW2Plan {
    int64_t elements = 0;   // basic elements of the origin
    int64_t bytes = 0;      // data bytes of the origin
    int path = 0;           // 0 nothing to do, 1 - 2 as in msx.h
    int64_t od = 0, td = 0; // where the origin's / target's one piece starts (path 1)
};
int dt_accw2_plan(int opidx, const Dtype* origin_t, int64_t origin_count, const Dtype* target_t,
                  int64_t target_count, AccW2Plan* plan);
int dt_accw2_dev(int opidx, const Dtype* origin_t, const void* origin, const Dtype* target_t, void* target,
                 const AccW2Plan& plan, hipStream_t s);

// msx_accumulate_batch_dev (msx.h): nseg independent msx_accumulate_dev calls of
// one builtin op in as few launches as possible.  dt_acc2_batch_plan runs the
// call's checks 6 and 7 (dt_acc2_plan per segment in index order, then one
// element kind for an op) and says what the call does with every non-empty
// segment: a segment below acc2_batch_fuse_below() data bytes whose two
// instance sizes the 32-bit address map can hold is fused, up to
// acc2_batch_width() per launch of msx_acc2_segs.hip's kernels, whatever its
// dt_acc2_plan path; every other one is dt_acc2_dev's.  dt_acc2_batch_dev does
// exactly that, in index order.
struct Acc2BatchStep {
    int seg = 0;
    const Dtype* ot = nullptr;
    const Dtype* tt = nullptr;
    int64_t ocount = 0;
    Acc2Plan plan;
    bool fused = false;
};
struct Acc2BatchPlan {
    std::vector<Acc2BatchStep> steps;   // the non-empty segments, in index order
    int fused = 0, single = 0;
    int launches() const;
};
int acc2_batch_width();
int64_t acc2_batch_fuse_below();
int dt_acc2_batch_plan(int opidx, const Dtype* const* origin_t, const int64_t* origin_count,
                       const Dtype* const* target_t, const int64_t* target_count, int nseg, Acc2BatchPlan* plan);
int dt_acc2_batch_dev(int opidx, const Acc2BatchPlan& plan, const void* const* origin, void* const* target,
                      hipStream_t s);

// msx_get_accumulate_dev (msx.h): result elem e = target elem e, then target
// elem e = origin elem e (op) target elem e, over THREE type maps.
// dt_gacc3_plan runs the call's checks 4 - 6 on the host-side types (no GPU is
// touched); origin_t is null under MPI_NO_OP, where the result triple counts
// the elements.  dt_gacc3_dev does what the plan says: path 1 is the fetch
// kernel of msx_fetch.hip (the engine copy for MPI_NO_OP) on the three pieces,
// path 2 (MPI_NO_OP) dt_acc2_dev's typed -> typed copy target -> result, path 3
// the three-layout kernel of msx_acc3.hip.
struct Acc3Plan {
    int64_t elements = 0;   // basic elements of the call (n)
    int64_t bytes = 0;      // their data bytes
    int path = 0;           // 0 nothing to do, 1 - 3 as in msx.h
    int granule = 0;        // bytes one work item moves (16-byte aligned bases)
    int64_t od = 0, rd = 0, td = 0;   // where each side's one piece starts (path 1)
};
int dt_gacc3_plan(int opidx, const Dtype* origin_t, int64_t origin_count, const Dtype* result_t,
                  int64_t result_count, const Dtype* target_t, int64_t target_count, Acc3Plan* plan);
int dt_gacc3_dev(int opidx, const Dtype* origin_t, const void* origin, const Dtype* result_t,
                 int64_t result_count, void* result, const Dtype* target_t, void* target, const Acc3Plan& plan,
                 hipStream_t s);

}  // namespace msx
