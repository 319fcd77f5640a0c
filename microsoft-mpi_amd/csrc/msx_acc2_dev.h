// msx_acc2_dev.h — the element code of the two-layout datatype kernels, shared by
// msx_acc2.hip (one pair of layouts per launch, msx_accumulate_dev) and
// msx_acc2_segs.hip (many pairs per launch, msx_accumulate_batch_dev), so a
// segment of a fused launch gets the bytes its own launch would have given it.
//
// One tile is kUnroll x 64 consecutive elements of one call, run by one wave.
// A whole tile runs the unrolled bodies (no lane predicates); a tile cut by n,
// and every tile of a call too large for the 32-bit divisions, runs the serial
// loops.  The address map is msx_dtype_map.h's.  msx_acc2.hip uses acc2_elem,
// the serial tiles and make_launch2g from here and keeps its own copy of the
// whole-tile bodies (see its header); msx_acc2_segs.hip uses everything.
//
// Included by .hip units only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "msx_dev_ops.h"
#include "msx_dtype.h"
#include "msx_dtype_map.h"
#include "msx_kernels.h"

namespace msx {
namespace dev {

// target element (op)= origin element; acc_elem's two forms (msx_pack.hip).
template <int OP, class T, bool ALIGNED>
__device__ __forceinline__ void acc2_elem(char* t, const char* o)
{
    constexpr int E = (int)sizeof(T);
    if constexpr (ALIGNED) {
        T* tt = reinterpret_cast<T*>(t);
        *tt = Fn<OP>::apply(*tt, *reinterpret_cast<const T*>(o));
    } else {
        T x, y;
        __builtin_memcpy(&x, t, E);
        __builtin_memcpy(&y, o, E);
        x = Fn<OP>::apply(x, y);
        __builtin_memcpy(t, &x, E);
    }
}

// The elements of one lane, one after the other (not unrolled): the call's last
// workgroup when its tile is cut by n, and every workgroup of a call too large
// for the 32-bit divisions.
template <int OP, class T, bool ALIGNED, bool NARROW>
__device__ __forceinline__ void acc2_tile_serial(const CopyArgs& o, const CopyArgs& t, int64_t n, int64_t g0)
{
    constexpr int E = (int)sizeof(T);
#pragma unroll 1
    for (int u = 0; u < kUnroll; ++u) {
        const int64_t g = g0 + u * 64;
        if (g < n) acc2_elem<OP, T, ALIGNED>(t.typed + map_off<E, NARROW>(t, g), o.typed + map_off<E, NARROW>(o, g));
    }
}

// A whole tile of a narrow call: no lane predicates.
template <int OP, class T, bool ALIGNED>
__device__ __forceinline__ void acc2_tile_whole(const CopyArgs& o, const CopyArgs& t, int64_t g0)
{
    constexpr int E = (int)sizeof(T);
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

template <int G, bool NARROW>
__device__ __forceinline__ void copy2_tile_serial(const CopyArgs& o, const CopyArgs& t, int64_t n, int64_t g0)
{
    typedef typename GranT<G>::T T;
#pragma unroll 1
    for (int u = 0; u < kUnroll; ++u) {
        const int64_t g = g0 + u * 64;
        if (g < n)
            *reinterpret_cast<T*>(t.typed + map_off<G, NARROW>(t, g)) =
                *reinterpret_cast<const T*>(o.typed + map_off<G, NARROW>(o, g));
    }
}

// MPI_REPLACE, a whole tile of a narrow call: granule g of the origin's type
// map to granule g of the target's.
template <int G>
__device__ __forceinline__ void copy2_tile_whole(const CopyArgs& o, const CopyArgs& t, int64_t g0)
{
    typedef typename GranT<G>::T T;
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
// Both maps in granules of G bytes, and the launch shape of n granules.
struct Launch2 {
    CopyArgs o, t;
    int narrow;
    dim3 grid;
};

// A granule per side: element e of the call is granule e of the origin's map in
// Go bytes and granule e of the target's in Gt bytes (Go == Gt but for the
// widening accumulate of msx_widen.hip: 2-byte elements into 4-byte ones).
inline hipError_t make_launch2g(const DevLayout& Lo, const void* origin, int Go, const DevLayout& Lt, void* target,
                                int Gt, int64_t n, Launch2* l)
{
    // every run offset / length must hold whole granules for the granule map
    if (Lo.size % Go || Lt.size % Gt || (Lo.regular && Lo.blen % Go) || (Lt.regular && Lt.blen % Gt))
        return hipErrorInvalidValue;
    l->o = make_args(Lo, 1, const_cast<void*>(origin), nullptr, Go);
    l->t = make_args(Lt, 1, target, nullptr, Gt);
    // the 32-bit magic divisions hold for g, and every instance, below 2^32 granules
    l->narrow = dt_map_narrow(n, l->o.gsize, l->t.gsize);
    const int64_t tiles = (n + 64 * kUnroll - 1) / (64 * kUnroll);
    if (tiles > 0x7fffffffll) return hipErrorInvalidValue;     // > 2^39 elements: beyond any HBM
    l->grid = dim3((unsigned)tiles);
    return hipSuccess;
}

}  // namespace dev
}  // namespace msx
