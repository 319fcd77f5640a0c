// msx_combine_segs.hip — the multi-segment streaming combine: many independent
// `inout[i] = inout[i] (op) in[i]` operand pairs in one launch
// (msx_reduce_local_batch_dev), the combine's counterpart of k_copy_segs.
//
// The element code is msx_combine_dev.h's (combine_split, ld<>, issued_together,
// apply_vec, Fn<OP>::apply), so a segment's bytes are those of k_combine on the
// same operands.  One workgroup per 4-KiB tile (256 lanes x one 16-byte vector
// per operand) of one segment; the descriptors travel in the kernel arguments
// by value, as CopySegs does.  No LDS, no MFMA: the kernel is bandwidth-bound.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>

#include "msx_combine_dev.h"
#include "msx_kernels.h"
#include "msx_op_kind.h"

namespace msx {
namespace dev {

constexpr int kSegBlock = 256;

// 28 bytes per segment plus one closing prefix entry and the count: 3592 bytes
// at 128 segments, inside the 4-KiB kernel-argument block.
struct CombineSegs {
    const void* in[kCombineSegsWidth];
    void* io[kCombineSegsWidth];
    uint32_t count[kCombineSegsWidth];      // elements of T (below 16 MiB per operand)
    uint32_t head[kCombineSegsWidth];       // scalar elements before the vector body; == count: all scalar
    uint32_t tile0[kCombineSegsWidth + 1];  // exclusive prefix of the segments' tile counts
    int n;
};
static_assert(sizeof(CombineSegs) <= 4096, "descriptors must fit the kernel-argument block");

// Tile k of a segment: vectors [256k, 256k + 256) of its body and scalar
// elements [256k, 256k + 256) of its head + tail list, each guarded per lane.
// An aligned segment has at most 2 * (EPV - 1) scalars, all in tile 0; an
// all-scalar one (operands at different offsets from 16-byte alignment) has
// no vectors and count / 256 tiles.
template <int OP, class T, class VT>
__global__ __launch_bounds__(kSegBlock) void k_combine_segs(CombineSegs c)
{
    constexpr unsigned EPV = 16 / sizeof(T);
    // XCD x takes one contiguous eighth of the launch's tiles (xcd_tile)
    const unsigned t = xcd_tile(blockIdx.x, gridDim.x);
    // segment of tile t: the last sg with tile0[sg] <= t.  Wave-uniform (t
    // comes from blockIdx): scalar loads from the kernel arguments, at most
    // log2(width) = 7 steps, once per workgroup.
    int lo = 0, hi = c.n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (c.tile0[mid] <= t) lo = mid;
        else hi = mid;
    }
    const unsigned k = t - c.tile0[lo];
    const T* __restrict__ in = static_cast<const T*>(c.in[lo]);
    T* __restrict__ io = static_cast<T*>(c.io[lo]);
    const unsigned count = c.count[lo], head = c.head[lo];
    const unsigned nvec = (count - head) / EPV;
    const unsigned body_end = head + nvec * EPV;
    const unsigned v = k * kSegBlock + threadIdx.x;
    if (v < nvec) {
        const u32x4* __restrict__ vin = reinterpret_cast<const u32x4*>(in + head);
        u32x4* __restrict__ vio = reinterpret_cast<u32x4*>(io + head);
        u32x4 x = ld<true>(vin + v), y = ld<true>(vio + v);
        issued_together(x, y);      // both loads before the first use (msx_combine_dev.h)
        vio[v] = apply_vec<OP, VT>(y, x);
    }
    const unsigned nscalar = head + (count - body_end);
    if (v < nscalar) {
        const unsigned e = v < head ? v : body_end + (v - head);
        io[e] = Fn<OP>::apply(io[e], in[e]);
    }
}

}  // namespace dev

namespace {

using namespace dev;

template <int OP, class T, class VT>
hipError_t run_segs(const CombineSeg* segs, int nseg, size_t scale, hipStream_t s)
{
    CombineSegs c{};
    uint32_t tiles = 0;
    int n = 0;
    for (int i = 0; i < nseg; ++i) {
        const size_t count = segs[i].count * scale;
        if (count == 0) continue;
        if (count * sizeof(T) >= kCombineSegsMaxBytes || !segs[i].in || !segs[i].io) return hipErrorInvalidValue;
        size_t head, nvec, tail;
        combine_split<T>(segs[i].in, segs[i].io, count, head, nvec, tail);
        const size_t nt = std::max((nvec + kSegBlock - 1) / kSegBlock, (head + tail + kSegBlock - 1) / kSegBlock);
        c.in[n] = segs[i].in;
        c.io[n] = segs[i].io;
        c.count[n] = (uint32_t)count;
        c.head[n] = (uint32_t)head;
        c.tile0[n] = tiles;
        tiles += (uint32_t)nt;          // <= 128 segments x 65536 tiles
        ++n;
    }
    if (n == 0) return hipSuccess;
    for (int i = n; i <= kCombineSegsWidth; ++i) c.tile0[i] = tiles;
    c.n = n;
    hipLaunchKernelGGL((k_combine_segs<OP, T, VT>), dim3(tiles), dim3(kSegBlock), 0, s, c);
    return hipGetLastError();
}

template <int OP, class T>
hipError_t segs_default(const CombineSeg* g, int n, hipStream_t s) { return run_segs<OP, T, T>(g, n, 1, s); }

// Bitwise ops: byte-granular scalars, 32-bit lanes inside vectors (run_bitwise).
template <int OP>
hipError_t segs_bitwise(Kind k, const CombineSeg* g, int n, hipStream_t s)
{
    return run_segs<OP, uint8_t, uint32_t>(g, n, (size_t)kind_size(k), s);
}

}  // namespace

hipError_t launch_combine_segs(int opidx, Kind k, const CombineSeg* g, int n, hipStream_t s)
{
    if (n < 0 || n > kCombineSegsWidth || (n > 0 && !g)) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    return for_op(single_combine_op(opidx, k), [&](auto op) {
        constexpr int OP = decltype(op)::value;
        if constexpr (op_bytewise(OP))
            return segs_bitwise<OP>(k, g, n, s);
        else
            return for_kind<OP>(k, [&](auto t) { return segs_default<OP, typename decltype(t)::type>(g, n, s); });
    });
}

}  // namespace msx
