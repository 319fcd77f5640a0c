// msx_pack.hip — gfx950 kernels of the derived-datatype engine (msx_dtype.h).
//
// The reference interprets a dataloop tree on the CPU, one contiguous piece at
// a time (MPID_Segment_pack / unpack, mpid/segment.cpp; the accumulate walk of
// packethandling.cpp:2969-3004).  Here a committed type is a flat list of byte
// runs, and every work item maps one packed granule straight to its typed
// address:
//
//   packed byte p of instance i  ->  typed[i*extent + disp[k] + (p - poff[k])]
//
// with k found by a magic-number division for regular layouts (vector,
// hvector, subarray rows: run k = first + k*stride) and by a binary search
// over the run offsets otherwise (the map itself: msx_dtype_map.h, shared with
// the two-layout kernels of msx_acc2.hip).  The granule G is the largest power of two
// <= 16 that divides every run offset / length, the size, the extent and both
// pointers, so a granule never straddles two runs and every access is a
// naturally aligned G-byte load or store.  The kernels are HBM-bound byte
// movers (no arithmetic beyond the address map); a pack moves 2*size bytes per
// instance.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "msx_dev_ops.h"
#include "msx_dtype.h"
#include "msx_dtype_map.h"
#include "msx_kernels.h"
#include "msx_op_kind.h"

namespace msx {
namespace dev {

constexpr int kPackBlock = 256;

template <int G, bool REG, bool NARROW, bool UNPACK>
__global__ __launch_bounds__(kPackBlock) void k_dt_pack(CopyArgs a)
{
    typedef typename GranT<G>::T T;
    const int64_t stride = (int64_t)gridDim.x * kPackBlock;
    const int64_t bid = xcd_tile(blockIdx.x, gridDim.x);
    for (int64_t g0 = bid * kPackBlock + threadIdx.x; g0 < a.ngran; g0 += stride * kUnroll) {
        T v[kUnroll];
        int64_t off[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int64_t g = g0 + u * stride;
            if (g < a.ngran) {
                off[u] = typed_off<G, REG, NARROW>(a, g);
                if constexpr (UNPACK) v[u] = __builtin_nontemporal_load(reinterpret_cast<const T*>(a.packed) + g);
                else v[u] = *reinterpret_cast<const T*>(a.typed + off[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int64_t g = g0 + u * stride;
            if (g < a.ngran) {
                if constexpr (UNPACK) *reinterpret_cast<T*>(a.typed + off[u]) = v[u];
                else __builtin_nontemporal_store(v[u], reinterpret_cast<T*>(a.packed) + g);
            }
        }
    }
}

// Tile form for spans far above the 256 MiB Infinity Cache (the combine's
// DRAM-regime geometry, k_combine_dram): one-wave workgroups in dispatch
// order, each owning kUnroll x 64 consecutive granules, so the eight XCDs
// stream neighbouring tiles of both sides instead of the grid-stride form's
// 4 x 8 streams per side.  Same map, loads before stores, same cache policy.
template <int G, bool REG, bool NARROW, bool UNPACK>
__global__ __launch_bounds__(64) void k_dt_pack_tile(CopyArgs a)
{
    typedef typename GranT<G>::T T;
    const int64_t g0 = (int64_t)blockIdx.x * (64 * kUnroll) + threadIdx.x;
    T v[kUnroll];
    int64_t off[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
        const int64_t g = g0 + u * 64;
        if (g < a.ngran) {
            off[u] = typed_off<G, REG, NARROW>(a, g);
            if constexpr (UNPACK) v[u] = __builtin_nontemporal_load(reinterpret_cast<const T*>(a.packed) + g);
            else v[u] = *reinterpret_cast<const T*>(a.typed + off[u]);
        }
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
        const int64_t g = g0 + u * 64;
        if (g < a.ngran) {
            if constexpr (UNPACK) *reinterpret_cast<T*>(a.typed + off[u]) = v[u];
            else __builtin_nontemporal_store(v[u], reinterpret_cast<T*>(a.packed) + g);
        }
    }
}

// Run-parallel form for layouts whose runs are long (subarray rows, big
// indexed blocks): one wavefront per (instance, run) unit, its 64 lanes
// stream the run's granules with coalesced accesses on both sides.  No
// per-granule search: the run's offsets are read once per wave.
template <int G, bool UNPACK>
__global__ __launch_bounds__(kPackBlock) void k_dt_runs(CopyArgs a)
{
    typedef typename GranT<G>::T T;
    constexpr int kWaves = kPackBlock / 64;
    const int lane = threadIdx.x & 63;
    const int64_t nunits = (a.ngran / a.gsize) * a.nruns;        // instances x runs
    const int64_t nw = (int64_t)gridDim.x * kWaves;
    // (dispatch order here: XCD-contiguous order measured 10 % slower for this kernel)
    for (int64_t u = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); u < nunits; u += nw) {
        const int64_t i = u / a.nruns, k = u - i * a.nruns;
        int64_t po, len, disp;
        if (a.n1) {             // two-level regular layout: run k computed, no tables
            const int64_t k1 = k / a.n1;
            po = k * a.gblen * G;
            len = a.gblen;
            disp = a.first + k1 * a.stride2 + (k - k1 * a.n1) * a.stride;
        } else {
            po = a.poff[k];
            len = (a.poff[k + 1] - po) / G;
            disp = a.disp[k];
        }
        T* t = reinterpret_cast<T*>(a.typed + i * a.extent + disp);
        T* p = reinterpret_cast<T*>(a.packed + i * a.size + po);
        for (int64_t j0 = lane; j0 < len; j0 += 64 * kUnroll) {
            T v[kUnroll];
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                const int64_t j = j0 + 64 * u;
                if (j < len) {
                    if constexpr (UNPACK) v[u] = __builtin_nontemporal_load(p + j);
                    else v[u] = t[j];
                }
            }
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                const int64_t j = j0 + 64 * u;
                if (j < len) {
                    if constexpr (UNPACK) t[j] = v[u];
                    else __builtin_nontemporal_store(v[u], p + j);
                }
            }
        }
    }
}

// typed element (op)= packed element.  E = element bytes; granules are whole
// elements.  ALIGNED: every element address is a multiple of alignof(T);
// otherwise the element moves through byte copies.
template <int OP, class T, bool ALIGNED>
__device__ __forceinline__ void acc_elem(char* t, const char* p)
{
    constexpr int E = (int)sizeof(T);
    if constexpr (ALIGNED) {
        T* tt = reinterpret_cast<T*>(t);
        *tt = Fn<OP>::apply(*tt, *reinterpret_cast<const T*>(p));
    } else {
        T x, y;
        __builtin_memcpy(&x, t, E);
        __builtin_memcpy(&y, p, E);
        x = Fn<OP>::apply(x, y);
        __builtin_memcpy(t, &x, E);
    }
}

// The derived-target accumulate, in the pack kernels' tile form
// (k_dt_pack_tile): one-wave workgroups in dispatch order, kUnroll x 64
// consecutive elements each, every operand of the tile loaded before the first
// combine when the elements are aligned.  (Rounds 2-5 also carried a
// grid-stride form; the tile form beat it at every size measured, below.)
template <int OP, class T, bool REG, bool ALIGNED>
__global__ __launch_bounds__(64) void k_dt_acc_tile(CopyArgs a)
{
    constexpr int E = (int)sizeof(T);
    const int64_t g0 = (int64_t)blockIdx.x * (64 * kUnroll) + threadIdx.x;
    if constexpr (ALIGNED) {
        T x[kUnroll], y[kUnroll];
        T* tt[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int64_t g = g0 + u * 64;
            if (g < a.ngran) {
                tt[u] = reinterpret_cast<T*>(a.typed + typed_off<E, REG, false>(a, g));
                x[u] = *tt[u];
                y[u] = reinterpret_cast<const T*>(a.packed)[g];
            }
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u)
            if (g0 + u * 64 < a.ngran) *tt[u] = Fn<OP>::apply(x[u], y[u]);
    } else {
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int64_t g = g0 + u * 64;
            if (g < a.ngran) acc_elem<OP, T, false>(a.typed + typed_off<E, REG, false>(a, g), a.packed + g * E);
        }
    }
}

// ---- host side ---------------------------------------------------------------
int grid_for(int64_t n)
{
    // a few waves of workgroups over 256 CUs; the loops are grid-stride
    const int64_t want = (n + kPackBlock - 1) / kPackBlock;
    return (int)(want < 8192 ? (want > 0 ? want : 1) : 8192);
}

// Average run length (in granules) from which a wave per run beats the
// per-granule binary search.
constexpr int64_t kRunParallelMin = 8;

}  // namespace dev

// Pack/unpack geometry (msx_tune_pack): 0 = by size (the tile form when the
// call's typed span plus packed bytes exceed pack_tile_min()), 1 = always the
// grid-stride form, 2 = always the tile form.
int g_pack_mode = 0;

constexpr size_t kPackTileMin = (size_t)512 << 20;
size_t pack_tile_min() { return kPackTileMin; }

// A derived-target accumulate always runs k_dt_acc_tile.  Self-targeted fp32
// SUM MPI_Accumulate through a 16-B-block vector target type, grid-stride ->
// tile form, three interleaved rounds (round 3,
// profiles/r03/acc_geometry/): 256 MiB window 144 -> 140 us per call, 1 GiB
// 663 -> 521 us.

int pack_tune_set(int mode)
{
    if (mode < 0 || mode > 2) return -1;
    g_pack_mode = mode;
    return 0;
}

namespace dev {

template <int G, bool UNPACK>
hipError_t run_copy(const CopyArgs& a, bool reg, hipStream_t s)
{
    const bool narrow = a.ngran < (int64_t)0xffffffffll;
    const dim3 block(kPackBlock);
    // Two-level regular layouts (2-D / 3-D subarrays) map granules by two
    // magic-number divisions in the tile form, which beats the wave-per-run
    // kernel at every size measured (3-D fp32 subarray, 1536-B rows, runs ->
    // tile: 256 MiB pack 35.0 -> 34.3 us, unpack 37.7 -> 37.1; 2 GiB pack
    // 348.5 -> 313.5, unpack 378.4 -> 347.4; scripts/pack_size_probe.py,
    // profiles/r03/pack_geometry/).  msx_tune_pack 1 keeps the wave-per-run
    // kernel for them, 2 forces the tile form for every layout.
    const bool two_level = reg && a.n1 != 0;
    const bool tile_first = g_pack_mode == 2 || (g_pack_mode == 0 && two_level);
    // long runs: irregular tables, or a two-level regular layout under mode 1
    if (!tile_first && (!reg || a.n1) && a.gsize >= kRunParallelMin * a.nruns) {
        const int64_t units = (a.ngran / a.gsize) * a.nruns;
        const int64_t want = (units + kPackBlock / 64 - 1) / (kPackBlock / 64);
        const dim3 grid((unsigned)(want < 8192 ? want : 8192));
        hipLaunchKernelGGL((k_dt_runs<G, UNPACK>), grid, block, 0, s, a);
        return hipGetLastError();
    }
    const size_t span = (size_t)(a.ngran / a.gsize) * (size_t)a.extent + (size_t)a.ngran * G;
    if (tile_first || (g_pack_mode == 0 && span > pack_tile_min())) {
        const int64_t want = (a.ngran + 64 * kUnroll - 1) / (64 * kUnroll);
        if (want <= 0x7fffffffll) {
            const dim3 tg((unsigned)want), tb(64);
            if (reg && narrow) hipLaunchKernelGGL((k_dt_pack_tile<G, true, true, UNPACK>), tg, tb, 0, s, a);
            else if (reg) hipLaunchKernelGGL((k_dt_pack_tile<G, true, false, UNPACK>), tg, tb, 0, s, a);
            else hipLaunchKernelGGL((k_dt_pack_tile<G, false, false, UNPACK>), tg, tb, 0, s, a);
            return hipGetLastError();
        }
    }
    const dim3 grid(grid_for(a.ngran));
    if (reg && narrow) hipLaunchKernelGGL((k_dt_pack<G, true, true, UNPACK>), grid, block, 0, s, a);
    else if (reg) hipLaunchKernelGGL((k_dt_pack<G, true, false, UNPACK>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((k_dt_pack<G, false, false, UNPACK>), grid, block, 0, s, a);
    return hipGetLastError();
}

template <bool UNPACK>
hipError_t copy_g(int G, const CopyArgs& a, bool reg, hipStream_t s)
{
    return for_granule(G, [&](auto g) { return run_copy<decltype(g)::value, UNPACK>(a, reg, s); });
}

// One (op, element type) pair of msx_op_kind.h's map.
template <int OP, class T>
hipError_t run_acc(const DevLayout& L, int64_t count, const void* packed, void* typed, hipStream_t s)
{
    constexpr int E = (int)sizeof(T);
    // every run offset / length must hold whole elements for the element map
    if (L.size % E) return hipErrorInvalidValue;
    CopyArgs a = make_args(L, count, typed, const_cast<void*>(packed), E);
    if (L.regular && (L.blen % E)) return hipErrorInvalidValue;
    const bool aligned = L.align >= (int)alignof(T);
    const bool reg = L.regular != 0;
    const int64_t tiles = (a.ngran + 64 * kUnroll - 1) / (64 * kUnroll);
    if (tiles == 0) return hipSuccess;
    if (tiles > 0x7fffffffll) return hipErrorInvalidValue;     // > 2^39 elements: beyond any HBM
    const dim3 tg((unsigned)tiles), tb(64);
    if (reg && aligned) hipLaunchKernelGGL((k_dt_acc_tile<OP, T, true, true>), tg, tb, 0, s, a);
    else if (reg) hipLaunchKernelGGL((k_dt_acc_tile<OP, T, true, false>), tg, tb, 0, s, a);
    else if (aligned) hipLaunchKernelGGL((k_dt_acc_tile<OP, T, false, true>), tg, tb, 0, s, a);
    else hipLaunchKernelGGL((k_dt_acc_tile<OP, T, false, false>), tg, tb, 0, s, a);
    return hipGetLastError();
}

}  // namespace dev

hipError_t launch_dt_copy(const DevLayout& L, int64_t count, void* typed, void* packed, bool unpack,
                          hipStream_t s)
{
    if (count <= 0 || L.size == 0) return hipSuccess;
    const int G = L.align;
    if (G < 1 || G > 16 || (G & (G - 1)) || L.size % G || (L.regular && L.blen % G))
        return hipErrorInvalidValue;
    dev::CopyArgs a = dev::make_args(L, count, typed, packed, G);
    return unpack ? dev::copy_g<true>(G, a, L.regular != 0, s) : dev::copy_g<false>(G, a, L.regular != 0, s);
}

hipError_t launch_dt_acc(int opidx, Kind k, const DevLayout& L, int64_t count, const void* packed,
                         void* typed, hipStream_t s)
{
    if (count <= 0 || L.size == 0) return hipSuccess;
    if (opidx == O_REPLACE) return launch_dt_copy(L, count, typed, const_cast<void*>(packed), true, s);
    return for_op(opidx, [&](auto op) {
        return for_kind<decltype(op)::value>(k, [&](auto t) {
            return dev::run_acc<decltype(op)::value, typename decltype(t)::type>(L, count, packed, typed, s);
        });
    });
}

}  // namespace msx
