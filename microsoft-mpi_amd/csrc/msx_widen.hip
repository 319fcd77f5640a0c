// msx_widen.hip — gfx950 kernels of msx_accumulate_widen_dev (msx.h): 16-bit
// float origins (MSX_FLOAT16, MSX_BFLOAT16) combined into fp32 targets,
//   target[e] = F_op(target[e], W(origin[e]))
// in ONE launch, for contiguous operands (the streaming kernels) and for any
// two committed layouts (the two-layout kernels).
//
// Without it the operation is a conversion pass into an fp32 scratch buffer
// and msx_reduce_local_dev on MPI_FLOAT: two launches, a scratch buffer and 18
// bytes of traffic per element against the 10 (2 + 4 read, 4 written) moved
// here; strided operands had no route without packing first.
//
// Streaming kernels: the combine's two geometries (msx_kernels.hip) over work
// items of 8 elements.  Up to combine_dram_min() bytes of the TARGET (the
// larger operand; which operand to hold against the bound is not measured):
// 256-lane XCD-contiguous tiles, non-temporal loads, plain stores.  Above it:
// one-wave workgroups in XCD runs of kDramRun tiles, non-temporal loads, sc1
// store.  Both policies are the combine's in the same regime, taken over and
// not measured for this kernel's 10-byte mix.  Lane assignment: lane i takes
// target vectors i and i + BLOCK of its tile and two 8-byte origin loads, so
// every instruction is fully coalesced (widen_body, msx_widen_dev.h).  The body
// and the operand split are msx_widen_dev.h's.  A unit of its own, so the
// combine's code objects stay as they are.
//
// Two-layout kernels: k_dt_acc2_tile's geometry and three forms (msx_acc2.hip)
// with a granule per side: element e is granule e of the origin's map in
// 2-byte granules and granule e of the target's in 4-byte granules.  A
// contiguous side is a layout of one run.  No __restrict__: the two spans may
// interleave.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "msx_acc2_dev.h"
#include "msx_dtype.h"
#include "msx_dtype_map.h"
#include "msx_kernels.h"
#include "msx_op_kind.h"
#include "msx_widen_dev.h"

namespace msx {
namespace dev {

// ---- contiguous operands --------------------------------------------------------
template <int OP, class H, int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_widen_combine(const uint16_t* in, uint32_t* io, size_t head, size_t nvec,
                                                         size_t tail)
{
    widen_body<OP, H, BLOCK, 0, FlagPolicy<true, false>>(in, io, head, nvec, tail);
}

template <int OP, class H, int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_widen_combine_dram(const uint16_t* in, uint32_t* io, size_t head,
                                                              size_t nvec, size_t tail)
{
    widen_body<OP, H, BLOCK, kDramRun, DramPolicy<true>>(in, io, head, nvec, tail);
}

// Operands off their natural alignment (origin % 2, target % 4): byte copies,
// one element per lane, grid-stride.
template <int OP, class H, int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_widen_combine_bytes(const char* in, char* io, size_t n)
{
    for (size_t e = (size_t)blockIdx.x * BLOCK + threadIdx.x; e < n; e += (size_t)gridDim.x * BLOCK)
        widen_elem<OP, H, false>(io + 4 * e, in + 2 * e);
}

// ---- two layouts ----------------------------------------------------------------
template <int OP, class H, bool ALIGNED, bool NARROW>
__device__ __forceinline__ void accw2_tile_serial(const CopyArgs& o, const CopyArgs& t, int64_t n, int64_t g0)
{
#pragma unroll 1
    for (int u = 0; u < kUnroll; ++u) {
        const int64_t g = g0 + u * 64;
        if (g < n) widen_elem<OP, H, ALIGNED>(t.typed + map_off<4, NARROW>(t, g), o.typed + map_off<2, NARROW>(o, g));
    }
}

// o.typed / t.typed: the origin and target buffer addresses; n elements.
template <int OP, class H, bool ALIGNED>
__global__ __launch_bounds__(64) void k_dt_accw2_tile(CopyArgs o, CopyArgs t, int64_t n, int narrow)
{
    const int64_t g0 = (int64_t)blockIdx.x * (64 * kUnroll) + threadIdx.x;
    if (!narrow) return accw2_tile_serial<OP, H, ALIGNED, false>(o, t, n, g0);
    if ((int64_t)(blockIdx.x + 1) * (64 * kUnroll) > n) return accw2_tile_serial<OP, H, ALIGNED, true>(o, t, n, g0);
    // a whole tile: no lane predicates
    if constexpr (ALIGNED) {
        // every address first, then the operand loads, then the stores
        int64_t to[kUnroll], oo[kUnroll];
        uint32_t x[kUnroll] = {};
        uint16_t y[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            to[u] = map_off<4, true>(t, g0 + u * 64);
            oo[u] = map_off<2, true>(o, g0 + u * 64);
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            if constexpr (OP != O_REPLACE) x[u] = *reinterpret_cast<const uint32_t*>(t.typed + to[u]);
            y[u] = *reinterpret_cast<const uint16_t*>(o.typed + oo[u]);
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u)
            *reinterpret_cast<uint32_t*>(t.typed + to[u]) = widen_apply<OP>(x[u], widen_bits<H>(y[u]));
    } else {
#pragma unroll
        for (int u = 0; u < kUnroll; ++u)
            widen_elem<OP, H, false>(t.typed + map_off<4, true>(t, g0 + u * 64),
                                     o.typed + map_off<2, true>(o, g0 + u * 64));
    }
}

// ---- host side ------------------------------------------------------------------
// run_fetch's launch shapes (msx_fetch.hip) over 8-element work items.
template <int OP, class H>
hipError_t run_widen(const void* in, void* io, size_t count, hipStream_t s)
{
    constexpr int BLOCK = 256, DB = 64;
    if (((uintptr_t)in & 1) || ((uintptr_t)io & 3)) {
        size_t grid = (count + BLOCK - 1) / BLOCK;
        if (grid > 0x7fffffffu) grid = 0x7fffffffu;
        hipLaunchKernelGGL((k_widen_combine_bytes<OP, H, BLOCK>), dim3((unsigned)grid), dim3(BLOCK), 0, s,
                           static_cast<const char*>(in), static_cast<char*>(io), count);
        return hipGetLastError();
    }
    size_t head, nvec, tail;
    widen_split(in, io, count, head, nvec, tail);
    if (nvec * 32 > combine_dram_min()) {
        size_t grid = (nvec + DB - 1) / DB;
        const size_t sc = (head + tail + DB - 1) / DB;
        if (grid < sc) grid = sc;
        if (grid > 0x7fffffffu) return hipErrorInvalidValue;    // > 2^38 target bytes
        hipLaunchKernelGGL((k_widen_combine_dram<OP, H, DB>), dim3((unsigned)grid), dim3(DB), 0, s,
                           static_cast<const uint16_t*>(in), static_cast<uint32_t*>(io), head, nvec, tail);
        return hipGetLastError();
    }
    size_t grid = (nvec + BLOCK - 1) / BLOCK;
    const size_t sc = (head + tail + BLOCK - 1) / BLOCK;
    if (grid < sc) grid = sc;
    if (grid == 0) return hipSuccess;
    if (grid > 0x7fffffffu) grid = 0x7fffffffu;
    hipLaunchKernelGGL((k_widen_combine<OP, H, BLOCK>), dim3((unsigned)grid), dim3(BLOCK), 0, s,
                       static_cast<const uint16_t*>(in), static_cast<uint32_t*>(io), head, nvec, tail);
    return hipGetLastError();
}

template <int OP, class H>
hipError_t run_accw2(const DevLayout& Lo, const void* origin, const DevLayout& Lt, void* target, int64_t n,
                     bool aligned, hipStream_t s)
{
    Launch2 l;
    const hipError_t e = make_launch2g(Lo, origin, 2, Lt, target, 4, n, &l);
    if (e != hipSuccess) return e;
    if (aligned)
        hipLaunchKernelGGL((k_dt_accw2_tile<OP, H, true>), l.grid, dim3(64), 0, s, l.o, l.t, n, l.narrow);
    else
        hipLaunchKernelGGL((k_dt_accw2_tile<OP, H, false>), l.grid, dim3(64), 0, s, l.o, l.t, n, l.narrow);
    return hipGetLastError();
}

// f(OpTag<OP>{}, TypeTag<H>{}) for the ten (op, 16-bit kind) pairs of the call.
template <class F>
hipError_t for_widen(int opidx, Kind k, F&& f)
{
    auto with_op = [&](auto t) {
        switch (opidx) {
        case O_SUM:     return f(OpTag<O_SUM>{}, t);
        case O_PROD:    return f(OpTag<O_PROD>{}, t);
        case O_MAX:     return f(OpTag<O_MAX>{}, t);
        case O_MIN:     return f(OpTag<O_MIN>{}, t);
        case O_REPLACE: return f(OpTag<O_REPLACE>{}, t);
        default:        return hipErrorInvalidValue;
        }
    };
    if (k == K_F16) return with_op(TypeTag<f16>{});
    if (k == K_BF16) return with_op(TypeTag<bf16>{});
    return hipErrorInvalidValue;
}

}  // namespace dev

hipError_t launch_widen_combine(int opidx, Kind k, const void* in, void* inout, size_t n, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    return dev::for_widen(opidx, k, [&](auto op, auto t) {
        return dev::run_widen<decltype(op)::value, typename decltype(t)::type>(in, inout, n, s);
    });
}

hipError_t launch_dt_accw2(int opidx, Kind k, const DevLayout& Lo, const void* origin, const DevLayout& Lt,
                           void* target, int64_t n, bool aligned, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    return dev::for_widen(opidx, k, [&](auto op, auto t) {
        return dev::run_accw2<decltype(op)::value, typename decltype(t)::type>(Lo, origin, Lt, target, n, aligned, s);
    });
}

}  // namespace msx
