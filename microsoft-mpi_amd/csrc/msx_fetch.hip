// msx_fetch.hip — gfx950 kernels of msx_fetch_and_op_dev (msx.h): the streaming
// combine that also hands back the old `inout`,
//   fetched[i] = inout[i];  inout[i] = inout[i] (op) in[i]
// in ONE launch.
//
// The reference reaches this through a window only: MPI_Fetch_and_op /
// MPI_Get_accumulate copy the target's old value into the result buffer and
// then call MPID_Uop_call(origin, target) on it
// (Handle_MPIDI_CH3_PKT_GET_ACCUMULATE, packethandling.cpp:2121, and its
// receive handlers).  On device operands that is a copy launch (2 N
// bytes) followed by a combine launch (3 N); here each tile's `inout` vector is
// loaded once and stored twice, so the call moves 4 N bytes.
//
// Geometry, cache policy of the three combine streams and the operand split
// are the combine's (msx_kernels.hip: k_combine up to combine_dram_min(),
// k_combine_dram above it); the body is fetch_body of msx_combine_dev.h.  A
// unit of its own, so the combine's code objects stay as they are.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "msx_combine_dev.h"
#include "msx_kernels.h"
#include "msx_op_kind.h"

namespace msx {
namespace dev {

// Up to combine_dram_min(): k_combine's 256-lane XCD-contiguous tiles,
// non-temporal loads, plain stores on both outputs.
template <int OP, class T, class VT, int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_fetch_combine(const T* __restrict__ in, T* __restrict__ io,
                                                         T* __restrict__ fo, size_t head, size_t nvec, size_t tail)
{
    fetch_body<OP, T, VT, 1, BLOCK, 0, FlagPolicy<true, false>, StPol::plain>(in, io, fo, head, nvec, tail);
}

// Above it: k_combine_dram's one-wave workgroups in XCD runs of kDramRun
// tiles, non-temporal loads, sc1 store of `inout`, and a non-temporal store of
// `fetched` (kFetchDramSt).  Picked from the probe library's candidates in this
// geometry (k_probe_fetch_pol), timed interleaved with the two calls the kernel
// replaces (scripts/fetch_combine_probe.py, 256 MiB fp32 SUM per operand, 5
// rounds, us back to back / cache flushed, profiles/fetch/policy_sc1_build.json;
// that build's product kernel stored `fetched` sc1 and measured as the sc1 row):
//   fetched store   plain          nt             sc1            sc0 sc1
//                   187.3 / 186.2  151.2 / 170.2  180.7 / 180.5  180.3 / 179.5
//   copy + combine (two launches, 5 N bytes)      202.5 / 214.7
// sc1 on both stores was the starting guess because `inout`'s store has it; the
// non-temporal store is 16 % ahead of it back to back and 6 % cache flushed,
// beyond the 1 - 2 % spreads.  A second record with this policy in the product
// (profiles/fetch/fetch_combine.json, another machine, everything ~10 % faster)
// has nt 147.0 / 168.2 against sc1 164.5 / 165.6: 11 % ahead back to back again,
// cache flushed inside the spreads.  Only this size was measured.
template <int OP, class T, class VT, int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_fetch_combine_dram(const T* __restrict__ in, T* __restrict__ io,
                                                              T* __restrict__ fo, size_t head, size_t nvec,
                                                              size_t tail)
{
    fetch_dram_body<OP, T, VT, BLOCK>(in, io, fo, head, nvec, tail);
}

}  // namespace dev

namespace {

using namespace dev;

// run_combine's launch shapes (msx_kernels.hip) without its realigning and
// host-operand forms.
template <int OP, class T, class VT>
hipError_t run_fetch(const void* in, void* io, void* fo, size_t count, hipStream_t s)
{
    constexpr int BLOCK = 256, DB = 64;
    size_t head, nvec, tail;
    fetch_split<T>(in, io, fo, count, head, nvec, tail);
    if (nvec * 16 > combine_dram_min()) {
        size_t grid = (nvec + DB - 1) / DB;
        const size_t sc = (head + tail + DB - 1) / DB;
        if (grid < sc) grid = sc;
        if (grid > 0x7fffffffu) return hipErrorInvalidValue;    // > 2^37 bytes per operand
        hipLaunchKernelGGL((k_fetch_combine_dram<OP, T, VT, DB>), dim3((unsigned)grid), dim3(DB), 0, s,
                           static_cast<const T*>(in), static_cast<T*>(io), static_cast<T*>(fo), head, nvec, tail);
        return hipGetLastError();
    }
    size_t grid = (nvec + BLOCK - 1) / BLOCK;
    const size_t sc = (head + tail + BLOCK - 1) / BLOCK;
    if (grid < sc) grid = sc;
    if (grid == 0) return hipSuccess;
    if (grid > 0x7fffffffu) grid = 0x7fffffffu;
    hipLaunchKernelGGL((k_fetch_combine<OP, T, VT, BLOCK>), dim3((unsigned)grid), dim3(BLOCK), 0, s,
                       static_cast<const T*>(in), static_cast<T*>(io), static_cast<T*>(fo), head, nvec, tail);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_fetch_combine(int opidx, Kind k, const void* in, void* fetched, void* inout, size_t n,
                                hipStream_t s)
{
    if (n == 0) return hipSuccess;
    // MPI_REPLACE moves bytes: one byte-wise instantiation, 32-bit lanes in the vectors
    if (opidx == O_REPLACE) return run_fetch<O_REPLACE, uint8_t, uint32_t>(in, inout, fetched, n * kind_size(k), s);
    return for_op(single_combine_op(opidx, k), [&](auto op) {
        constexpr int OP = decltype(op)::value;
        if constexpr (op_bytewise(OP))
            return run_fetch<OP, uint8_t, uint32_t>(in, inout, fetched, n * kind_size(k), s);
        else
            return for_kind<OP>(k, [&](auto t) {
                using T = typename decltype(t)::type;
                return run_fetch<OP, T, T>(in, inout, fetched, n, s);
            });
    });
}

}  // namespace msx
