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

// The (op, kind) set of launch_combine's switch (msx_kernels.hip).
template <int OP>
hipError_t segs_arith(Kind k, const CombineSeg* g, int n, hipStream_t s)
{
    switch (k) {
    case K_I8:  return segs_default<OP, int8_t>(g, n, s);
    case K_U8:  return segs_default<OP, uint8_t>(g, n, s);
    case K_I16: return segs_default<OP, int16_t>(g, n, s);
    case K_U16: return segs_default<OP, uint16_t>(g, n, s);
    case K_I32: return segs_default<OP, int32_t>(g, n, s);
    case K_U32: return segs_default<OP, uint32_t>(g, n, s);
    case K_I64: return segs_default<OP, int64_t>(g, n, s);
    case K_U64: return segs_default<OP, uint64_t>(g, n, s);
    case K_F32: return segs_default<OP, float>(g, n, s);
    case K_F64: return segs_default<OP, double>(g, n, s);
    default: break;
    }
    if constexpr (OP == O_SUM || OP == O_PROD) {
        if (k == K_C32) return segs_default<OP, c32>(g, n, s);
        if (k == K_C64) return segs_default<OP, c64>(g, n, s);
    }
    if constexpr (OP == O_LAND || OP == O_LOR || OP == O_LXOR) {
        if (k == K_BOOL) return segs_default<OP, uint8_t>(g, n, s);
    }
    if constexpr (OP == O_SUM || OP == O_PROD || OP == O_MAX || OP == O_MIN) {
        if (k == K_F16) return segs_default<OP, f16>(g, n, s);
        if (k == K_BF16) return segs_default<OP, bf16>(g, n, s);
    }
    return hipErrorInvalidValue;
}

template <int OP>
hipError_t segs_loc(Kind k, const CombineSeg* g, int n, hipStream_t s)
{
    switch (k) {
    case K_LOC_II: return segs_default<OP, loc_ii>(g, n, s);
    case K_LOC_FI: return segs_default<OP, loc_fi>(g, n, s);
    case K_LOC_SI: return segs_default<OP, loc_si>(g, n, s);
    case K_LOC_DI: return segs_default<OP, loc_di>(g, n, s);
    case K_LOC_FF: return segs_default<OP, loc_ff>(g, n, s);
    case K_LOC_DD: return segs_default<OP, loc_dd>(g, n, s);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace

hipError_t launch_combine_segs(int opidx, Kind k, const CombineSeg* g, int n, hipStream_t s)
{
    if (n < 0 || n > kCombineSegsWidth || (n > 0 && !g)) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    switch (opidx) {
    case O_SUM_WIDE:   // one combine: MPI_SUM's kernel, as launch_combine
        if (k != K_F16 && k != K_BF16) return hipErrorInvalidValue;
        return segs_arith<O_SUM>(k, g, n, s);
    case O_SUM:  return segs_arith<O_SUM>(k, g, n, s);
    case O_MAX:  return segs_arith<O_MAX>(k, g, n, s);
    case O_MIN:  return segs_arith<O_MIN>(k, g, n, s);
    case O_PROD: return segs_arith<O_PROD>(k, g, n, s);
    case O_LAND: return segs_arith<O_LAND>(k, g, n, s);
    case O_LOR:  return segs_arith<O_LOR>(k, g, n, s);
    case O_LXOR: return segs_arith<O_LXOR>(k, g, n, s);
    case O_BAND: return segs_bitwise<O_BAND>(k, g, n, s);
    case O_BOR:  return segs_bitwise<O_BOR>(k, g, n, s);
    case O_BXOR: return segs_bitwise<O_BXOR>(k, g, n, s);
    case O_MAXLOC: return segs_loc<O_MAXLOC>(k, g, n, s);
    case O_MINLOC: return segs_loc<O_MINLOC>(k, g, n, s);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace msx
