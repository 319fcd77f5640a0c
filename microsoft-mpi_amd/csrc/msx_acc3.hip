// msx_acc3.hip — gfx950 kernels of msx_get_accumulate_dev (msx.h): fetch and
// combine between THREE datatype layouts, none of them packed.
//
//   result[e] = target[e];  target[e] = origin[e] (op) target[e]      e < n
//
// The reference reaches this through a window: MPI_Get_accumulate ships the
// packed origin, the target side copies its old elements into a response and
// then walks its dataloop calling MPID_Uop_call(origin, target)
// (Handle_MPIDI_CH3_PKT_GET_ACCUMULATE, packethandling.cpp:2121; win.cpp:1804),
// and the origin unpacks the response into the result triple.  Here element e
// is mapped straight to its address on all three sides by the O(1) map of
// msx_dtype_map.h, so the call moves its own 4 N bytes in one launch and needs
// no scratch; msx_accumulate_dev twice (a 2 N copy, then a 3 N combine) moves
// 5 N in two.
//
// Geometry and forms are msx_acc2.hip's: one-wave workgroups in dispatch order,
// kUnroll x 64 consecutive elements each; "regular or irregular layout" is a
// wave-uniform run-time branch per side; in the aligned form a lane computes
// its 3 * kUnroll addresses, issues its 2 * kUnroll loads, then stores.  The
// serial form (a loop that is not unrolled) runs the call's last workgroup when
// n cuts its tile and every workgroup of a call of 2^32 elements or more, or
// with an instance of 2^32 granules.  Two kernels per (op, element type) pair
// (aligned, unaligned) whatever the three layouts are, and one exchange kernel
// per granule for MPI_REPLACE.
//
// No __restrict__ on the kernels' operands: the spans may interleave (result
// and target two columns of one matrix).  Each lane reads element e of the
// origin and of the target before it stores element e of the result and of the
// target, and no other lane touches element e of any side.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "msx_dev_ops.h"
#include "msx_dtype.h"
#include "msx_dtype_map.h"
#include "msx_kernels.h"
#include "msx_op_kind.h"

namespace msx {
namespace dev {

// result element = target element (whole: a pair struct's padding too), then
// target element (op)= origin element; acc2_elem's two forms.
template <int OP, class T, bool ALIGNED>
__device__ __forceinline__ void gacc3_elem(char* r, char* t, const char* o)
{
    constexpr int E = (int)sizeof(T);
    if constexpr (ALIGNED) {
        T* tt = reinterpret_cast<T*>(t);
        const T x = *tt, y = *reinterpret_cast<const T*>(o);
        *reinterpret_cast<T*>(r) = x;
        *tt = Fn<OP>::apply(x, y);
    } else {
        T x, y;
        __builtin_memcpy(&x, t, E);
        __builtin_memcpy(&y, o, E);
        __builtin_memcpy(r, &x, E);
        x = Fn<OP>::apply(x, y);
        __builtin_memcpy(t, &x, E);
    }
}

template <int OP, class T, bool ALIGNED, bool NARROW>
__device__ __forceinline__ void gacc3_tile_serial(const CopyArgs& o, const CopyArgs& r, const CopyArgs& t, int64_t n,
                                                  int64_t g0)
{
    constexpr int E = (int)sizeof(T);
#pragma unroll 1
    for (int u = 0; u < kUnroll; ++u) {
        const int64_t g = g0 + u * 64;
        if (g < n)
            gacc3_elem<OP, T, ALIGNED>(r.typed + map_off<E, NARROW>(r, g), t.typed + map_off<E, NARROW>(t, g),
                                       o.typed + map_off<E, NARROW>(o, g));
    }
}

// o.typed / r.typed / t.typed: the origin, result and target buffer addresses; n elements.
template <int OP, class T, bool ALIGNED>
__global__ __launch_bounds__(64) void k_dt_gacc3_tile(CopyArgs o, CopyArgs r, CopyArgs t, int64_t n, int narrow)
{
    constexpr int E = (int)sizeof(T);
    const int64_t g0 = (int64_t)blockIdx.x * (64 * kUnroll) + threadIdx.x;
    if (!narrow) return gacc3_tile_serial<OP, T, ALIGNED, false>(o, r, t, n, g0);
    if ((int64_t)(blockIdx.x + 1) * (64 * kUnroll) > n) return gacc3_tile_serial<OP, T, ALIGNED, true>(o, r, t, n, g0);
    // a whole tile: no lane predicates
    if constexpr (ALIGNED) {
        int64_t to[kUnroll], ro[kUnroll], oo[kUnroll];
        T x[kUnroll], y[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            to[u] = map_off<E, true>(t, g0 + u * 64);
            ro[u] = map_off<E, true>(r, g0 + u * 64);
            oo[u] = map_off<E, true>(o, g0 + u * 64);
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            x[u] = *reinterpret_cast<const T*>(t.typed + to[u]);
            y[u] = *reinterpret_cast<const T*>(o.typed + oo[u]);
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            *reinterpret_cast<T*>(r.typed + ro[u]) = x[u];
            *reinterpret_cast<T*>(t.typed + to[u]) = Fn<OP>::apply(x[u], y[u]);
        }
    } else {
#pragma unroll
        for (int u = 0; u < kUnroll; ++u)
            gacc3_elem<OP, T, false>(r.typed + map_off<E, true>(r, g0 + u * 64), t.typed + map_off<E, true>(t, g0 + u * 64),
                                     o.typed + map_off<E, true>(o, g0 + u * 64));
    }
}

template <int G, bool NARROW>
__device__ __forceinline__ void xchg3_tile_serial(const CopyArgs& o, const CopyArgs& r, const CopyArgs& t, int64_t n,
                                                  int64_t g0)
{
    typedef typename GranT<G>::T T;
#pragma unroll 1
    for (int u = 0; u < kUnroll; ++u) {
        const int64_t g = g0 + u * 64;
        if (g < n) {
            T* tp = reinterpret_cast<T*>(t.typed + map_off<G, NARROW>(t, g));
            const T x = *tp, y = *reinterpret_cast<const T*>(o.typed + map_off<G, NARROW>(o, g));
            *reinterpret_cast<T*>(r.typed + map_off<G, NARROW>(r, g)) = x;
            *tp = y;
        }
    }
}

// MPI_REPLACE: granule g of the target's type map goes to granule g of the
// result's, granule g of the origin's to the target's; G the largest granule
// the three layouts and the three pointers allow.
template <int G>
__global__ __launch_bounds__(64) void k_dt_xchg3_tile(CopyArgs o, CopyArgs r, CopyArgs t, int64_t n, int narrow)
{
    typedef typename GranT<G>::T T;
    const int64_t g0 = (int64_t)blockIdx.x * (64 * kUnroll) + threadIdx.x;
    if (!narrow) return xchg3_tile_serial<G, false>(o, r, t, n, g0);
    if ((int64_t)(blockIdx.x + 1) * (64 * kUnroll) > n) return xchg3_tile_serial<G, true>(o, r, t, n, g0);
    int64_t to[kUnroll], ro[kUnroll], oo[kUnroll];
    T x[kUnroll], y[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
        to[u] = map_off<G, true>(t, g0 + u * 64);
        ro[u] = map_off<G, true>(r, g0 + u * 64);
        oo[u] = map_off<G, true>(o, g0 + u * 64);
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
        x[u] = *reinterpret_cast<const T*>(t.typed + to[u]);
        y[u] = *reinterpret_cast<const T*>(o.typed + oo[u]);
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
        *reinterpret_cast<T*>(r.typed + ro[u]) = x[u];
        *reinterpret_cast<T*>(t.typed + to[u]) = y[u];
    }
}

// ---- host side ---------------------------------------------------------------
// The three maps in granules of G bytes, and the launch shape of n granules.
struct Launch3 {
    CopyArgs o, r, t;
    int narrow;
    dim3 grid;
};

static hipError_t make_launch3(const DevLayout& Lo, const void* origin, const DevLayout& Lr, void* result,
                               const DevLayout& Lt, void* target, int64_t n, int G, Launch3* l)
{
    // every run offset / length must hold whole granules for the granule map
    for (const DevLayout* L : {&Lo, &Lr, &Lt})
        if (L->size % G || (L->regular && L->blen % G)) return hipErrorInvalidValue;
    l->o = make_args(Lo, 1, const_cast<void*>(origin), nullptr, G);
    l->r = make_args(Lr, 1, result, nullptr, G);
    l->t = make_args(Lt, 1, target, nullptr, G);
    // the 32-bit magic divisions hold for g, and every instance, below 2^32 granules
    l->narrow = dt_map_narrow(n, l->o.gsize, l->t.gsize, l->r.gsize);
    const int64_t tiles = (n + 64 * kUnroll - 1) / (64 * kUnroll);
    if (tiles > 0x7fffffffll) return hipErrorInvalidValue;     // > 2^39 elements: beyond any HBM
    l->grid = dim3((unsigned)tiles);
    return hipSuccess;
}

// One (op, element type) pair of msx_op_kind.h's map.
template <int OP, class T>
hipError_t run_gacc3(const DevLayout& Lo, const void* origin, const DevLayout& Lr, void* result, const DevLayout& Lt,
                     void* target, int64_t n, int align, hipStream_t s)
{
    Launch3 l;
    const hipError_t e = make_launch3(Lo, origin, Lr, result, Lt, target, n, (int)sizeof(T), &l);
    if (e != hipSuccess) return e;
    if (align >= (int)alignof(T))
        hipLaunchKernelGGL((k_dt_gacc3_tile<OP, T, true>), l.grid, dim3(64), 0, s, l.o, l.r, l.t, n, l.narrow);
    else
        hipLaunchKernelGGL((k_dt_gacc3_tile<OP, T, false>), l.grid, dim3(64), 0, s, l.o, l.r, l.t, n, l.narrow);
    return hipGetLastError();
}

template <int G>
hipError_t run_xchg3(const DevLayout& Lo, const void* origin, const DevLayout& Lr, void* result, const DevLayout& Lt,
                     void* target, int64_t n, hipStream_t s)
{
    Launch3 l;
    const hipError_t e = make_launch3(Lo, origin, Lr, result, Lt, target, n, G, &l);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_dt_xchg3_tile<G>), l.grid, dim3(64), 0, s, l.o, l.r, l.t, n, l.narrow);
    return hipGetLastError();
}

}  // namespace dev

// result element e = target element e, then target element e (op)= origin
// element e, for e < n; elements of kind k in type-map order of the three
// layouts.  align: the largest power of two dividing every element address of
// the three sides (layouts and pointers).
hipError_t launch_dt_gacc3(int opidx, Kind k, const DevLayout& Lo, const void* origin, const DevLayout& Lr,
                           void* result, const DevLayout& Lt, void* target, int64_t n, int align, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    return for_op(opidx, [&](auto op) {
        return for_kind<decltype(op)::value>(k, [&](auto t) {
            return dev::run_gacc3<decltype(op)::value, typename decltype(t)::type>(Lo, origin, Lr, result, Lt, target, n,
                                                                                  align, s);
        });
    });
}

// The first `bytes` data bytes of the target's type map to the result's and of
// the origin's to the target's, in granules of G bytes (a power of two <= 16
// dividing the three layouts' run offsets and lengths, the three pointers and
// `bytes`).
hipError_t launch_dt_xchg3(const DevLayout& Lo, const void* origin, const DevLayout& Lr, void* result,
                           const DevLayout& Lt, void* target, int64_t bytes, int G, hipStream_t s)
{
    if (bytes <= 0) return hipSuccess;
    if (G < 1 || G > 16 || (G & (G - 1)) || bytes % G) return hipErrorInvalidValue;
    const int64_t n = bytes / G;
    return for_granule(G, [&](auto g) {
        return dev::run_xchg3<decltype(g)::value>(Lo, origin, Lr, result, Lt, target, n, s);
    });
}

}  // namespace msx
