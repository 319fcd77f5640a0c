// msx_acc2.hip — gfx950 kernels of msx_accumulate_dev (msx.h): a combine and a
// copy between TWO datatype layouts, neither side packed.
//
// The reference reaches this through a window: MPI_Accumulate packs the origin,
// ships it, and the target walks its dataloop calling MPID_Uop_call(origin,
// target) piece by piece (win.cpp:1435, packethandling.cpp:2969-3004); its
// typed -> typed MPIR_Localcopy (pt2pt.cpp:770-948) packs into a bounce buffer
// and unpacks from it.  Here element e of the call is mapped straight to its
// address on BOTH sides by the O(1) map of msx_dtype_map.h, so the operation
// moves its own 3 N bytes (N for a copy's read, N for its write) in one launch
// and needs no scratch.
//
// Geometry: k_dt_acc_tile's (msx_pack.hip).  One-wave workgroups in dispatch
// order, kUnroll x 64 consecutive elements each; in the aligned form a lane
// issues its 2 * kUnroll loads before its first store.  "Regular or irregular
// layout" is a wave-uniform run-time branch per side (CopyArgs::poff is a
// kernel argument), not a template parameter, so each (op, element type) pair
// costs two kernels (aligned, unaligned) whatever the two layouts are.  Two
// cases run a lane's elements one after the other in a loop that is not
// unrolled, to keep the kernels small: the call's last workgroup when n cuts
// its tile (so the unrolled form carries no lane predicates), and calls of 2^32
// elements or more, or with an instance of 2^32 granules, which divide in 64
// bits (cold: 4 Gi elements is 4 GiB of int8).
//
// No __restrict__ on the kernels' operands: the two spans may interleave (two
// columns of one matrix).  Each lane reads element e of both sides before it
// stores it, and no other lane touches element e.
//
// acc2_elem, the serial tiles and the launch shape (make_launch2g) are
// msx_acc2_dev.h's, shared with msx_acc2_segs.hip.  The whole-tile bodies stay
// written out in the two kernels here: calling msx_acc2_dev.h's
// acc2_tile_whole / copy2_tile_whole instead gives the same instructions in
// another register assignment, and these kernels' machine code is kept as it
// was (scripts/compare_kernels.py).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "msx_acc2_dev.h"
#include "msx_dev_ops.h"
#include "msx_dtype.h"
#include "msx_dtype_map.h"
#include "msx_kernels.h"
#include "msx_op_kind.h"

namespace msx {
namespace dev {

// o.typed / t.typed: the origin and target buffer addresses; n elements.
template <int OP, class T, bool ALIGNED>
__global__ __launch_bounds__(64) void k_dt_acc2_tile(CopyArgs o, CopyArgs t, int64_t n, int narrow)
{
    constexpr int E = (int)sizeof(T);
    const int64_t g0 = (int64_t)blockIdx.x * (64 * kUnroll) + threadIdx.x;
    if (!narrow) return acc2_tile_serial<OP, T, ALIGNED, false>(o, t, n, g0);
    if ((int64_t)(blockIdx.x + 1) * (64 * kUnroll) > n) return acc2_tile_serial<OP, T, ALIGNED, true>(o, t, n, g0);
    // a whole tile: no lane predicates
    if constexpr (ALIGNED) {
        // every address first (an irregular side's table search waits for its
        // own loads only), then the 2 * kUnroll operand loads, then the stores
        int64_t to[kUnroll], oo[kUnroll];
        T x[kUnroll], y[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            to[u] = map_off<E, true>(t, g0 + u * 64);
            oo[u] = map_off<E, true>(o, g0 + u * 64);
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            x[u] = *reinterpret_cast<const T*>(t.typed + to[u]);
            y[u] = *reinterpret_cast<const T*>(o.typed + oo[u]);
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) *reinterpret_cast<T*>(t.typed + to[u]) = Fn<OP>::apply(x[u], y[u]);
    } else {
#pragma unroll
        for (int u = 0; u < kUnroll; ++u)
            acc2_elem<OP, T, false>(t.typed + map_off<E, true>(t, g0 + u * 64), o.typed + map_off<E, true>(o, g0 + u * 64));
    }
}

// MPI_REPLACE: granule g of the origin's type map to granule g of the
// target's, G the largest granule both layouts and both pointers allow.
template <int G>
__global__ __launch_bounds__(64) void k_dt_copy2_tile(CopyArgs o, CopyArgs t, int64_t n, int narrow)
{
    typedef typename GranT<G>::T T;
    const int64_t g0 = (int64_t)blockIdx.x * (64 * kUnroll) + threadIdx.x;
    if (!narrow) return copy2_tile_serial<G, false>(o, t, n, g0);
    if ((int64_t)(blockIdx.x + 1) * (64 * kUnroll) > n) return copy2_tile_serial<G, true>(o, t, n, g0);
    int64_t to[kUnroll], oo[kUnroll];
    T v[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
        to[u] = map_off<G, true>(t, g0 + u * 64);
        oo[u] = map_off<G, true>(o, g0 + u * 64);
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) v[u] = *reinterpret_cast<const T*>(o.typed + oo[u]);
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) *reinterpret_cast<T*>(t.typed + to[u]) = v[u];
}

// ---- host side ---------------------------------------------------------------
// One (op, element type) pair of msx_op_kind.h's map.
template <int OP, class T>
hipError_t run_acc2(const DevLayout& Lo, const void* origin, const DevLayout& Lt, void* target, int64_t n, int align,
                    hipStream_t s)
{
    Launch2 l;
    const hipError_t e = make_launch2g(Lo, origin, (int)sizeof(T), Lt, target, (int)sizeof(T), n, &l);
    if (e != hipSuccess) return e;
    if (align >= (int)alignof(T))
        hipLaunchKernelGGL((k_dt_acc2_tile<OP, T, true>), l.grid, dim3(64), 0, s, l.o, l.t, n, l.narrow);
    else
        hipLaunchKernelGGL((k_dt_acc2_tile<OP, T, false>), l.grid, dim3(64), 0, s, l.o, l.t, n, l.narrow);
    return hipGetLastError();
}

template <int G>
hipError_t run_copy2(const DevLayout& Lo, const void* origin, const DevLayout& Lt, void* target, int64_t n,
                     hipStream_t s)
{
    Launch2 l;
    const hipError_t e = make_launch2g(Lo, origin, G, Lt, target, G, n, &l);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_dt_copy2_tile<G>), l.grid, dim3(64), 0, s, l.o, l.t, n, l.narrow);
    return hipGetLastError();
}

}  // namespace dev

// target element e (op)= origin element e for e < n, elements of kind k in
// type-map order of the two layouts.  align: the largest power of two dividing
// every element address of both sides (layouts and pointers).
hipError_t launch_dt_acc2(int opidx, Kind k, const DevLayout& Lo, const void* origin, const DevLayout& Lt,
                          void* target, int64_t n, int align, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    return for_op(opidx, [&](auto op) {
        return for_kind<decltype(op)::value>(k, [&](auto t) {
            return dev::run_acc2<decltype(op)::value, typename decltype(t)::type>(Lo, origin, Lt, target, n, align, s);
        });
    });
}

// The first `bytes` data bytes of the origin's type map to the target's, in
// granules of G bytes (a power of two <= 16 dividing both layouts' run offsets
// and lengths, both pointers and `bytes`).
hipError_t launch_dt_copy2(const DevLayout& Lo, const void* origin, const DevLayout& Lt, void* target,
                           int64_t bytes, int G, hipStream_t s)
{
    if (bytes <= 0) return hipSuccess;
    if (G < 1 || G > 16 || (G & (G - 1)) || bytes % G) return hipErrorInvalidValue;
    const int64_t n = bytes / G;
    return for_granule(G, [&](auto g) { return dev::run_copy2<decltype(g)::value>(Lo, origin, Lt, target, n, s); });
}

}  // namespace msx
