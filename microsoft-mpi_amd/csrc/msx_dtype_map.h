// msx_dtype_map.h — the O(1) address map of a committed datatype layout, shared
// by the datatype kernels' units (msx_pack.hip: one typed side and a packed
// stream; msx_acc2.hip: a typed layout on both sides; msx_acc3.hip: on all
// three operands of a get-accumulate).
//
//   packed byte p of instance i  ->  typed[i*extent + disp[k] + (p - poff[k])]
//
// with k found by a magic-number division for regular layouts (vector,
// hvector, subarray rows: run k = first + k*stride) and by a binary search
// over the run offsets otherwise; msx_pack.hip's header has the whole story.
//
// Included by .hip units only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "msx_dev_ops.h"
#include "msx_dtype.h"

namespace msx {
namespace dev {

// q = n / d for any 32-bit n (Granlund-Montgomery round-up method).
struct FastDiv {
    uint32_t d = 1, m = 0, s = 0;
    FastDiv() = default;
    explicit FastDiv(uint32_t div) : d(div)
    {
        s = 0;
        while ((1ull << s) < div) ++s;
        m = (uint32_t)((((1ull << 32) * ((1ull << s) - div)) / div) + 1);
    }
    __device__ __forceinline__ uint32_t div(uint32_t n) const
    {
        return (uint32_t)(((uint64_t)__umulhi(n, m) + n) >> s);
    }
};

struct CopyArgs {
    char* typed;
    char* packed;
    int64_t ngran;           // granules in the packed stream (count * size / G)
    int64_t extent;          // bytes
    int64_t size;            // bytes per instance
    // regular layout, in granules where noted
    int64_t first;           // bytes
    int64_t stride;          // bytes
    int64_t gsize, gblen;    // granules
    FastDiv fd_size, fd_blen;
    // two-level regular layout (n1 > 0): run k at first + (k / n1)*stride2 + (k % n1)*stride
    int64_t n1, stride2;
    FastDiv fd_n1;
    // general layout
    const int64_t* disp;
    const int64_t* poff;
    int64_t nruns;
};

template <int G> struct GranT;
template <> struct GranT<1> { typedef uint8_t T; };
template <> struct GranT<2> { typedef uint16_t T; };
template <> struct GranT<4> { typedef uint32_t T; };
template <> struct GranT<8> { typedef uint64_t T; };
template <> struct GranT<16> { typedef u32x4 T; };

// Largest k with poff[k] <= q (poff[0] = 0, poff[nruns] = size > q).
__device__ __forceinline__ int64_t find_run(const int64_t* __restrict__ poff, int64_t nruns, int64_t q)
{
    int64_t lo = 0, hi = nruns;      // invariant: poff[lo] <= q < poff[hi]
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (poff[mid] <= q) lo = mid; else hi = mid;
    }
    return lo;
}

// Byte offset (from the typed base) of packed granule g.
template <int G, bool REG, bool NARROW>
__device__ __forceinline__ int64_t typed_off(const CopyArgs& a, int64_t g)
{
    int64_t i, q;
    if constexpr (NARROW) {
        const uint32_t gi = (uint32_t)a.fd_size.div((uint32_t)g);
        i = gi;
        q = g - (int64_t)gi * a.gsize;
    } else {
        i = g / a.gsize;
        q = g - i * a.gsize;
    }
    if constexpr (REG) {
        int64_t k;
        if constexpr (NARROW) k = a.fd_blen.div((uint32_t)q);
        else k = q / a.gblen;
        const int64_t off = q - k * a.gblen;
        if (a.n1) {             // two levels (uniform branch: a kernel argument)
            int64_t k1;
            if constexpr (NARROW) k1 = a.fd_n1.div((uint32_t)k);
            else k1 = k / a.n1;
            return i * a.extent + a.first + k1 * a.stride2 + (k - k1 * a.n1) * a.stride + off * G;
        }
        return i * a.extent + a.first + k * a.stride + off * G;
    } else {
        const int64_t qb = q * G;
        const int64_t k = find_run(a.poff, a.nruns, qb);
        return i * a.extent + a.disp[k] + (qb - a.poff[k]);
    }
}

// Byte offset of granule g in either kind of layout (the units with a layout on
// every side: msx_acc2.hip, msx_acc3.hip).
template <int G, bool NARROW>
__device__ __forceinline__ int64_t map_off(const CopyArgs& a, int64_t g)
{
    if (a.poff) return typed_off<G, false, NARROW>(a, g);      // uniform: a kernel argument
    return typed_off<G, true, NARROW>(a, g);
}

// Granules per lane in flight: every lane issues kUnroll independent loads
// before its first store (a lone load -> store chain per lane leaves too few
// bytes in flight per CU to cover HBM latency).
constexpr int kUnroll = 4;

// ---- host side ---------------------------------------------------------------
inline CopyArgs make_args(const DevLayout& L, int64_t count, void* typed, void* packed, int G)
{
    CopyArgs a{};
    a.typed = static_cast<char*>(typed);
    a.packed = static_cast<char*>(packed);
    a.extent = L.extent;
    a.size = L.size;
    a.gsize = L.size / G;
    a.ngran = count * a.gsize;
    a.nruns = L.nruns;
    if (L.regular) {
        a.first = L.first;
        a.stride = L.stride;
        a.gblen = L.blen / G;
        a.n1 = L.n1;
        a.stride2 = L.stride2;
    } else {
        a.disp = L.disp;
        a.poff = L.poff;
        a.nruns = L.nruns;
    }
    a.fd_size = FastDiv((uint32_t)(a.gsize < 0xffffffffll ? a.gsize : 1));
    a.fd_blen = FastDiv((uint32_t)(a.gblen > 0 && a.gblen < 0xffffffffll ? a.gblen : 1));
    a.fd_n1 = FastDiv((uint32_t)(a.n1 > 0 && a.n1 < 0xffffffffll ? a.n1 : 1));
    return a;
}

}  // namespace dev
}  // namespace msx
