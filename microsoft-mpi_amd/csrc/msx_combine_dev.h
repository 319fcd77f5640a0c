// msx_combine_dev.h — the streaming combine body `inout[i] = op(inout[i], in[i])`
// (src/mpi/msmpi/mpid/op.cpp:14-160 as an HBM stream).  Device code only;
// included by msx_kernels.hip (the product kernels), by msx_fetch.hip (the
// fetch form of the body, fetch_body below) and by the bench-only probe library
// (probe/msx_probe.hip), which times the same bodies under other symbols, in
// other tile orders and with other cache policies.
#pragma once

#include "msx_dev_ops.h"

namespace msx {
namespace dev {

// Both registers are inputs of one (empty) asm statement: their loads are
// issued back to back and waited for together, and no use of either can be
// scheduled between them.
__device__ __forceinline__ void issued_together(u32x4& x, u32x4& y)
{
    asm volatile("" : "+v"(x), "+v"(y));
    __builtin_amdgcn_sched_barrier(0);
}

// Tile order: 0 XCD-contiguous eighths, -1 dispatch order (round-robin over
// XCDs), G > 0 XCD x owns interleaved runs of G consecutive tiles.
template <int XG>
__device__ __forceinline__ size_t combine_tile(unsigned b, unsigned nb)
{
    if constexpr (XG == 0) {
        return xcd_tile(b, nb);
    } else if constexpr (XG < 0) {
        return b;
    } else {
        const unsigned full = (nb / (8u * XG)) * (8u * XG);
        if (b >= full) return b;
        const unsigned x = b & 7, j = b >> 3;
        return ((size_t)(j / XG) * 8 + x) * XG + (j % XG);
    }
}

// Cache policy of the body's three 16-byte streams.  `in` is never read again,
// the `inout` read is overwritten at once, the `inout` write is what the next
// combine on the same operands re-reads.  plain / nt are the global accesses
// of ld<> / st<>; the scope-bit forms (sc1: bypasses L1 on a load, drops the
// line from the XCD's L2 on a store) are raw buffer accesses.
enum class LdPol { plain, nt, sc1, sc1_nt };
enum class StPol { plain, nt, sc1, sc0_sc1 };
template <LdPol IN, LdPol IO, StPol ST>
struct CombinePolicy {
    static constexpr LdPol in = IN, io = IO;
    static constexpr StPol st = ST;
};
// What the two flags of the launchers have always meant.
template <bool NTLD, bool NTST>
using FlagPolicy = CombinePolicy<NTLD ? LdPol::nt : LdPol::plain, NTLD ? LdPol::nt : LdPol::plain,
                                 NTST ? StPol::nt : StPol::plain>;

// Buffer offsets are 32-bit: the resource is rebased on each tile (`tile`,
// workgroup-uniform, so it stays in scalar registers) and `off` is the lane's
// byte offset inside the tile, so operands of any size work.  `p` is the same
// address as a pointer, for the global forms.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t tile_rsrc(const u32x4* tile)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<u32x4*>(tile), 0, (int)0xFFFFFFFF, 0x00020000);
}
template <LdPol P>
__device__ __forceinline__ u32x4 ld_pol(const u32x4* p, const u32x4* tile, unsigned off)
{
    if constexpr (P == LdPol::plain) return ld<false>(p);
    else if constexpr (P == LdPol::nt) return ld<true>(p);
    else if constexpr (P == LdPol::sc1) return __builtin_amdgcn_raw_buffer_load_b128(tile_rsrc(tile), (int)off, 0, 16);
    else return __builtin_amdgcn_raw_buffer_load_b128(tile_rsrc(tile), (int)off, 0, 18);     // sc1 nt
}
template <StPol P>
__device__ __forceinline__ void st_pol(u32x4* p, u32x4* tile, unsigned off, u32x4 v)
{
    if constexpr (P == StPol::plain) st<false>(p, v);
    else if constexpr (P == StPol::nt) {
        // The value goes through an empty asm first: stored straight out of
        // apply_vec, the optimiser drops the store's non-temporal mark and
        // emits a plain global_store_dwordx4.
        asm volatile("" : "+v"(v));
        st<true>(p, v);
    }
    else if constexpr (P == StPol::sc1) __builtin_amdgcn_raw_buffer_store_b128(v, tile_rsrc(tile), (int)off, 0, 16);
    else __builtin_amdgcn_raw_buffer_store_b128(v, tile_rsrc(tile), (int)off, 0, 17);        // sc0 sc1
}

// Elements [0, head) and [head + nvec*EPV, head + nvec*EPV + tail) are scalar;
// the vector body starts at element `head`, 16-byte aligned for both operands.
// T  = element type used for scalar elements;
// VT = lane type used inside a 16-byte vector (== T except bitwise ops, which
//      run on 32-bit words regardless of the MPI element type).
// POL = cache policy of the full tiles' vector accesses; partial tiles and
//      scalar elements keep plain accesses.
template <int OP, class T, class VT, int UNROLL, int BLOCK, bool NTLD, bool NTST, int XG = 0,
          class POL = FlagPolicy<NTLD, NTST>>
__device__ __forceinline__ void combine_body(const T* __restrict__ in, T* __restrict__ io, size_t head,
                                             size_t nvec, size_t tail)
{
    constexpr size_t EPV = 16 / sizeof(T);
    constexpr size_t TILE = (size_t)BLOCK * UNROLL;
    const u32x4* __restrict__ vin = reinterpret_cast<const u32x4*>(in + head);
    u32x4* __restrict__ vio = reinterpret_cast<u32x4*>(io + head);
    const size_t bid = combine_tile<XG>(blockIdx.x, gridDim.x);

    for (size_t t0 = bid * TILE; t0 < nvec; t0 += (size_t)gridDim.x * TILE) {
        const size_t i0 = t0 + threadIdx.x;
        if (t0 + TILE <= nvec) {
            u32x4 a[UNROLL], b[UNROLL];
            const unsigned off0 = threadIdx.x * 16u;
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                a[u] = ld_pol<POL::in>(vin + i0 + (size_t)u * BLOCK, vin + t0, off0 + (unsigned)u * BLOCK * 16u);
                b[u] = ld_pol<POL::io>(vio + i0 + (size_t)u * BLOCK, vio + t0, off0 + (unsigned)u * BLOCK * 16u);
            }
            // Every load of the tile is issued before the first use: without
            // this the compiler hoists work on the first operand (logical ops,
            // complex, byte types) above the second load behind an
            // s_waitcnt vmcnt(0), halving the bytes in flight (-7..10 %).
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) issued_together(a[u], b[u]);
#pragma unroll
            for (int u = 0; u < UNROLL; ++u)
                st_pol<POL::st>(vio + i0 + (size_t)u * BLOCK, vio + t0, off0 + (unsigned)u * BLOCK * 16u,
                                apply_vec<OP, VT>(b[u], a[u]));
        } else {
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                const size_t i = i0 + (size_t)u * BLOCK;
                if (i < nvec) {
                    u32x4 x = vin[i], y = vio[i];
                    issued_together(x, y);
                    vio[i] = apply_vec<OP, VT>(y, x);
                }
            }
        }
    }

    const size_t nscalar = head + tail;
    if (nscalar) {
        const size_t body_end = head + nvec * EPV;
        for (size_t s = (size_t)blockIdx.x * BLOCK + threadIdx.x; s < nscalar;
             s += (size_t)gridDim.x * BLOCK) {
            const size_t e = s < head ? s : body_end + (s - head);
            io[e] = Fn<OP>::apply(io[e], in[e]);
        }
    }
}

// The product's DRAM-regime body (k_combine_dram, and the probe library's
// default_body_probe): UNROLL 1, XCD runs of kDramRun tiles, the launcher's
// load policy, and sc1 (write-through) stores whatever NTST says: the XCD's L2
// does not keep the written line, which nothing re-reads before a pass over
// all of both operands has gone through that L2 (table at k_combine_dram).
constexpr int kDramRun = 128;
template <bool NTLD>
using DramPolicy = CombinePolicy<NTLD ? LdPol::nt : LdPol::plain, NTLD ? LdPol::nt : LdPol::plain, StPol::sc1>;
template <int OP, class T, class VT, int BLOCK, bool NTLD, bool NTST>
__device__ __forceinline__ void combine_dram_body(const T* __restrict__ in, T* __restrict__ io, size_t head,
                                                  size_t nvec, size_t tail)
{
    combine_body<OP, T, VT, 1, BLOCK, NTLD, NTST, kDramRun, DramPolicy<NTLD>>(in, io, head, nvec, tail);
}

// ---- the fetch form (msx_fetch_and_op_dev, msx.h) ------------------------------
//   fetched[i] = inout[i]   (the old bytes, whole: a pair struct's padding too)
//   inout[i]   = inout[i] (op) in[i]
// combine_body with one more store per vector: the loaded `inout` vector goes to
// `fetched` as it came, then apply_vec's result to `inout`.  4 N bytes against
// the 2 N copy + 3 N combine of the two calls it replaces.  OP may also be
// O_REPLACE (inout[i] = in[i]), which has no functor: it moves bytes.
template <int OP, class VT>
__device__ __forceinline__ u32x4 fetch_apply_vec(u32x4 io, u32x4 in)
{
    if constexpr (OP == O_REPLACE) return in;
    else return apply_vec<OP, VT>(io, in);
}
template <int OP, class T>
__device__ __forceinline__ T fetch_apply(T io, T in)
{
    if constexpr (OP == O_REPLACE) return in;
    else return Fn<OP>::apply(io, in);
}

// POL: the combine's policy of its three streams; FST: the `fetched` store's.
// Partial tiles and scalar elements keep plain accesses, as in combine_body.
template <int OP, class T, class VT, int UNROLL, int BLOCK, int XG, class POL, StPol FST>
__device__ __forceinline__ void fetch_body(const T* __restrict__ in, T* __restrict__ io, T* __restrict__ fo,
                                           size_t head, size_t nvec, size_t tail)
{
    constexpr size_t EPV = 16 / sizeof(T);
    constexpr size_t TILE = (size_t)BLOCK * UNROLL;
    const u32x4* __restrict__ vin = reinterpret_cast<const u32x4*>(in + head);
    u32x4* __restrict__ vio = reinterpret_cast<u32x4*>(io + head);
    u32x4* __restrict__ vfo = reinterpret_cast<u32x4*>(fo + head);
    const size_t bid = combine_tile<XG>(blockIdx.x, gridDim.x);

    for (size_t t0 = bid * TILE; t0 < nvec; t0 += (size_t)gridDim.x * TILE) {
        const size_t i0 = t0 + threadIdx.x;
        if (t0 + TILE <= nvec) {
            u32x4 a[UNROLL], b[UNROLL];
            const unsigned off0 = threadIdx.x * 16u;
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                a[u] = ld_pol<POL::in>(vin + i0 + (size_t)u * BLOCK, vin + t0, off0 + (unsigned)u * BLOCK * 16u);
                b[u] = ld_pol<POL::io>(vio + i0 + (size_t)u * BLOCK, vio + t0, off0 + (unsigned)u * BLOCK * 16u);
            }
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) issued_together(a[u], b[u]);
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                st_pol<FST>(vfo + i0 + (size_t)u * BLOCK, vfo + t0, off0 + (unsigned)u * BLOCK * 16u, b[u]);
                st_pol<POL::st>(vio + i0 + (size_t)u * BLOCK, vio + t0, off0 + (unsigned)u * BLOCK * 16u,
                                fetch_apply_vec<OP, VT>(b[u], a[u]));
            }
        } else {
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                const size_t i = i0 + (size_t)u * BLOCK;
                if (i < nvec) {
                    u32x4 x = vin[i], y = vio[i];
                    issued_together(x, y);
                    vfo[i] = y;
                    vio[i] = fetch_apply_vec<OP, VT>(y, x);
                }
            }
        }
    }

    const size_t nscalar = head + tail;
    if (nscalar) {
        const size_t body_end = head + nvec * EPV;
        for (size_t s = (size_t)blockIdx.x * BLOCK + threadIdx.x; s < nscalar;
             s += (size_t)gridDim.x * BLOCK) {
            const size_t e = s < head ? s : body_end + (s - head);
            const T old = io[e];
            fo[e] = old;
            io[e] = fetch_apply<OP, T>(old, in[e]);
        }
    }
}

// The `fetched` store of the DRAM-regime fetch kernel (k_fetch_combine_dram and
// the probe library's default_fetch_probe): non-temporal.  Nothing in the call
// reads `fetched`, and a store that stays out of the caches leaves them to the
// two operands that are read; the table is at k_fetch_combine_dram.
constexpr StPol kFetchDramSt = StPol::nt;
template <int OP, class T, class VT, int BLOCK>
__device__ __forceinline__ void fetch_dram_body(const T* __restrict__ in, T* __restrict__ io, T* __restrict__ fo,
                                                size_t head, size_t nvec, size_t tail)
{
    fetch_body<OP, T, VT, 1, BLOCK, kDramRun, DramPolicy<true>, kFetchDramSt>(in, io, fo, head, nvec, tail);
}

// Operand split of the vector body: head scalars up to 16-byte alignment,
// whole 16-byte vectors, tail scalars.  Operands whose alignments disagree
// (or 16-byte elements off 16-byte alignment) are all-scalar here; the
// realigning kernel takes most of those (msx_kernels.hip, split_shift).
template <class T>
__host__ inline void combine_split(const void* in, const void* io, size_t count, size_t& head, size_t& nvec,
                                   size_t& tail)
{
    constexpr size_t ES = sizeof(T);
    const uintptr_t a = (uintptr_t)in, b = (uintptr_t)io;
    if ((a & 15) != (b & 15) || (a % ES) != 0 || (b % ES) != 0 || (ES == 16 && (a & 15))) {
        head = count; nvec = 0; tail = 0;
        return;
    }
    size_t h = ((16 - (a & 15)) & 15) / ES;
    if (h > count) h = count;
    const size_t rest = count - h;
    const size_t epv = 16 / ES;
    head = h; nvec = rest / epv; tail = rest - nvec * epv;
}

// combine_split for three operands: the vector body runs when all three share
// one offset from 16-byte alignment; otherwise the whole call is scalar (there
// is no realigning fetch kernel).
template <class T>
__host__ inline void fetch_split(const void* in, const void* io, const void* fo, size_t count, size_t& head,
                                 size_t& nvec, size_t& tail)
{
    if (((uintptr_t)fo & 15) != ((uintptr_t)io & 15) || ((uintptr_t)fo % sizeof(T)) != 0) {
        head = count; nvec = 0; tail = 0;
        return;
    }
    combine_split<T>(in, io, count, head, nvec, tail);
}

}  // namespace dev
}  // namespace msx
