// msx_acc2_segs.hip — the multi-segment two-layout combine: many independent
// `target[i] elem e (op)= origin[i] elem e` pairs of datatype layouts in one
// launch (msx_accumulate_batch_dev, msx.h), the typed counterpart of
// k_combine_segs.  A halo sum of a 3-D block is six such pairs of a few hundred
// KiB or less, each launch-bound on its own.
//
// The address map is msx_dtype_map.h's and the element code msx_acc2_dev.h's
// (acc2_elem, the serial tile, the whole-tile body), so a segment's bytes are
// those of k_dt_acc2_tile on the same operands.  Geometry: k_dt_acc2_tile's,
// one-wave workgroups of kUnroll x 64 consecutive elements of ONE segment; the
// tile -> segment step is a wave-uniform binary search over the exclusive
// prefix of the segments' tile counts, once per workgroup.  The descriptors
// (both address maps of every segment) travel in the kernel arguments by value,
// as CombineSegs does: no upload, no allocation, and the host arrays are free
// as soon as the launch is enqueued.  No LDS.  Only segments inside
// dt_map_narrow are fused, so the 64-bit form of the map is not instantiated.
//
// No __restrict__: the spans of a segment's two sides, and of different
// segments, may interleave (six faces of one array).  Each lane reads element
// e of both sides before it stores it, and no other lane of the launch touches
// a target element of that segment (msx.h's independence rule).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>

#include "msx_acc2_dev.h"
#include "msx_dev_ops.h"
#include "msx_dtype.h"
#include "msx_dtype_map.h"
#include "msx_kernels.h"
#include "msx_op_kind.h"

namespace msx {
namespace dev {

constexpr int kTile = 64 * kUnroll;

// Two unchanged CopyArgs (152 bytes each), the granule count and a prefix entry
// per segment: 3800 bytes at 12 segments, inside the 4-KiB kernel-argument block.
struct Acc2Segs {
    CopyArgs o[kAcc2SegsWidth];
    CopyArgs t[kAcc2SegsWidth];
    int64_t n[kAcc2SegsWidth];               // granules of the segment (below 2^32)
    uint32_t tile0[kAcc2SegsWidth + 1];      // exclusive prefix of the segments' tile counts
    int nseg;
};
static_assert(sizeof(Acc2Segs) <= 4096, "descriptors must fit the kernel-argument block");

// Segment of tile `tile`: the last sg with tile0[sg] <= tile.  Wave-uniform
// (blockIdx): scalar loads from the kernel arguments, at most 4 steps.
__device__ __forceinline__ int seg_of_tile(const Acc2Segs& c, unsigned tile)
{
    int lo = 0, hi = c.nseg;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (c.tile0[mid] <= tile) lo = mid;
        else hi = mid;
    }
    return lo;
}

template <int OP, class T, bool ALIGNED>
__global__ __launch_bounds__(64) void k_dt_acc2_segs(Acc2Segs c)
{
    const int sg = seg_of_tile(c, blockIdx.x);
    const unsigned k = blockIdx.x - c.tile0[sg];
    const CopyArgs& o = c.o[sg];
    const CopyArgs& t = c.t[sg];
    const int64_t n = c.n[sg];
    const int64_t g0 = (int64_t)k * kTile + threadIdx.x;
    if ((int64_t)(k + 1) * kTile > n) return acc2_tile_serial<OP, T, ALIGNED, true>(o, t, n, g0);
    acc2_tile_whole<OP, T, ALIGNED>(o, t, g0);
}

// MPI_REPLACE: granules of G bytes, G the smallest granule of the launch's segments.
template <int G>
__global__ __launch_bounds__(64) void k_dt_copy2_segs(Acc2Segs c)
{
    const int sg = seg_of_tile(c, blockIdx.x);
    const unsigned k = blockIdx.x - c.tile0[sg];
    const CopyArgs& o = c.o[sg];
    const CopyArgs& t = c.t[sg];
    const int64_t n = c.n[sg];
    const int64_t g0 = (int64_t)k * kTile + threadIdx.x;
    if ((int64_t)(k + 1) * kTile > n) return copy2_tile_serial<G, true>(o, t, n, g0);
    copy2_tile_whole<G>(o, t, g0);
}

// ---- host side ---------------------------------------------------------------
// The descriptors of one launch in granules of G bytes; *tiles its grid.
static hipError_t make_segs(const Acc2Seg* segs, int nseg, int G, Acc2Segs* c, uint32_t* tiles)
{
    *c = Acc2Segs();
    *tiles = 0;
    int n = 0;
    for (int i = 0; i < nseg; ++i) {
        const Acc2Seg& sg = segs[i];
        if (sg.bytes <= 0) continue;
        if (sg.bytes >= kAcc2SegsFuseBelow || sg.bytes % G || !sg.lo || !sg.lt || !sg.origin || !sg.target)
            return hipErrorInvalidValue;
        Launch2 l;
        const hipError_t e = make_launch2g(*sg.lo, sg.origin, G, *sg.lt, sg.target, G, sg.bytes / G, &l);
        if (e != hipSuccess) return e;
        if (!l.narrow) return hipErrorInvalidValue;       // the caller fuses narrow segments only
        c->o[n] = l.o;
        c->t[n] = l.t;
        c->n[n] = sg.bytes / G;
        c->tile0[n] = *tiles;
        *tiles += l.grid.x;                               // <= 12 segments x 65536 tiles
        ++n;
    }
    for (int i = n; i <= kAcc2SegsWidth; ++i) c->tile0[i] = *tiles;
    c->nseg = n;
    return hipSuccess;
}

static int min_align(const Acc2Seg* segs, int nseg)
{
    int a = 16;
    for (int i = 0; i < nseg; ++i)
        if (segs[i].bytes > 0) a = std::min(a, segs[i].align);
    return a;
}

// One (op, element type) pair of msx_op_kind.h's map.
template <int OP, class T>
hipError_t run_acc2_segs(const Acc2Seg* segs, int nseg, hipStream_t s)
{
    Acc2Segs c;
    uint32_t tiles;
    const hipError_t e = make_segs(segs, nseg, (int)sizeof(T), &c, &tiles);
    if (e != hipSuccess || tiles == 0) return e;
    // one misaligned address anywhere in the launch: the whole launch runs the unaligned form
    if (min_align(segs, nseg) >= (int)alignof(T))
        hipLaunchKernelGGL((k_dt_acc2_segs<OP, T, true>), dim3(tiles), dim3(64), 0, s, c);
    else
        hipLaunchKernelGGL((k_dt_acc2_segs<OP, T, false>), dim3(tiles), dim3(64), 0, s, c);
    return hipGetLastError();
}

template <int G>
hipError_t run_copy2_segs(const Acc2Seg* segs, int nseg, hipStream_t s)
{
    Acc2Segs c;
    uint32_t tiles;
    const hipError_t e = make_segs(segs, nseg, G, &c, &tiles);
    if (e != hipSuccess || tiles == 0) return e;
    hipLaunchKernelGGL((k_dt_copy2_segs<G>), dim3(tiles), dim3(64), 0, s, c);
    return hipGetLastError();
}

}  // namespace dev

hipError_t launch_dt_acc2_segs(int opidx, Kind k, const Acc2Seg* segs, int nseg, hipStream_t s)
{
    if (nseg < 0 || nseg > kAcc2SegsWidth || (nseg > 0 && !segs)) return hipErrorInvalidValue;
    if (nseg == 0) return hipSuccess;
    return for_op(opidx, [&](auto op) {
        return for_kind<decltype(op)::value>(k, [&](auto t) {
            return dev::run_acc2_segs<decltype(op)::value, typename decltype(t)::type>(segs, nseg, s);
        });
    });
}

hipError_t launch_dt_copy2_segs(const Acc2Seg* segs, int nseg, hipStream_t s)
{
    if (nseg < 0 || nseg > kAcc2SegsWidth || (nseg > 0 && !segs)) return hipErrorInvalidValue;
    if (nseg == 0) return hipSuccess;
    const int G = dev::min_align(segs, nseg);
    if (G < 1 || G > 16 || (G & (G - 1))) return hipErrorInvalidValue;
    return for_granule(G, [&](auto g) { return dev::run_copy2_segs<decltype(g)::value>(segs, nseg, s); });
}

}  // namespace msx
