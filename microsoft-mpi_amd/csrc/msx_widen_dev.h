// msx_widen_dev.h — device code of msx_accumulate_widen_dev (msx.h): a 16-bit
// float origin combined into an fp32 target,
//   target[e] = F_op(target[e], W(origin[e]))
// with F_op the fp32 functor Fn<OP>::apply(float, float) of msx_dev_ops.h (the
// x86 NaN rule for SUM / PROD, `inout > in ? inout : in` for MAX / MIN) and
// MPI_REPLACE the widening copy target[e] = W(origin[e]).
//
// W as bit patterns (uint16 x -> uint32): bf16 x << 16 for every x; fp16 the
// exact value of every non-NaN x (widen(), v_cvt_f32_f16, subnormals included)
// and, for a NaN, sign << 31 | 0x7F800000 | mantissa << 13 built in integers:
// payload and signalling state kept, whatever the convert instruction does
// with a signalling NaN.
//
// Included by msx_widen.hip only.
#pragma once

#include "msx_combine_dev.h"
#include "msx_dev_ops.h"

namespace msx {
namespace dev {

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

template <class H> __device__ __forceinline__ uint32_t widen_bits(uint16_t x);
template <> __device__ __forceinline__ uint32_t widen_bits<bf16>(uint16_t x) { return (uint32_t)x << 16; }
template <> __device__ __forceinline__ uint32_t widen_bits<f16>(uint16_t x)
{
    const uint32_t u = __float_as_uint(widen(f16{x}));
    const uint32_t nan = ((uint32_t)(x & 0x8000u) << 16) | 0x7F800000u | ((uint32_t)(x & 0x03FFu) << 13);
    return (x & 0x7FFFu) > 0x7C00u ? nan : u;
}

// One element: the new target value's bits from the old ones and W(origin).
template <int OP>
__device__ __forceinline__ uint32_t widen_apply(uint32_t io, uint32_t w)
{
    if constexpr (OP == O_REPLACE) return w;
    else return __float_as_uint(Fn<OP>::apply(__uint_as_float(io), __uint_as_float(w)));
}

// One 16-byte target vector and the four origin elements that go into it (two
// per 32-bit word, low half first).
template <int OP, class H>
__device__ __forceinline__ u32x4 widen_apply_vec(u32x4 io, u32x2 in)
{
    return u32x4{widen_apply<OP>(io.x, widen_bits<H>((uint16_t)in.x)),
                 widen_apply<OP>(io.y, widen_bits<H>((uint16_t)(in.x >> 16))),
                 widen_apply<OP>(io.z, widen_bits<H>((uint16_t)in.y)),
                 widen_apply<OP>(io.w, widen_bits<H>((uint16_t)(in.y >> 16)))};
}

template <bool NT>
__device__ __forceinline__ u32x2 ld8(const u32x2* p)
{
    if constexpr (NT) return __builtin_nontemporal_load(p);
    else return *p;
}

// The streaming body.  Elements [0, head) and [head + 8 nvec, head + 8 nvec +
// tail) are scalar; the vector body starts at element `head`, where both
// operands are 16-byte aligned, and covers nvec work items of 8 elements: one
// 16-byte origin vector and two 16-byte target vectors each.
//
// Lane assignment: a tile is BLOCK work items = 2 BLOCK target vectors, and
// lane i takes target vectors i and i + BLOCK of the tile with the two 8-byte
// origin halves that feed them.  Every load and store instruction of a wave
// then covers one contiguous range (512 B of the origin, 1 KiB of the target);
// with lane i on origin vector i and target vectors 2i, 2i + 1 each target
// instruction would touch every other 16 bytes of a 2-KiB range.  Chosen on
// that ground alone; the other assignment was not measured.
//
// As in combine_body: all of a tile's loads are issued before the first use,
// POL names the cache policy of the whole tiles' accesses (the 8-byte origin
// load is non-temporal unless POL::in is plain), partial tiles and scalar
// elements keep plain accesses.  MPI_REPLACE never reads the target.
template <int OP, class H, int BLOCK, int XG, class POL>
__device__ __forceinline__ void widen_body(const uint16_t* in, uint32_t* io, size_t head, size_t nvec, size_t tail)
{
    constexpr size_t TILE = (size_t)BLOCK * 2;
    constexpr bool NTIN = POL::in != LdPol::plain;
    const u32x2* vin = reinterpret_cast<const u32x2*>(in + head);
    u32x4* vio = reinterpret_cast<u32x4*>(io + head);
    const size_t nq = nvec * 2;                 // target vectors
    const size_t bid = combine_tile<XG>(blockIdx.x, gridDim.x);

    for (size_t t0 = bid * TILE; t0 < nq; t0 += (size_t)gridDim.x * TILE) {
        const size_t i0 = t0 + threadIdx.x;
        if (t0 + TILE <= nq) {
            u32x2 a[2];
            u32x4 b[2] = {};
            const unsigned off0 = threadIdx.x * 16u;
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                a[u] = ld8<NTIN>(vin + i0 + (size_t)u * BLOCK);
                if constexpr (OP != O_REPLACE)
                    b[u] = ld_pol<POL::io>(vio + i0 + (size_t)u * BLOCK, vio + t0, off0 + (unsigned)u * BLOCK * 16u);
            }
            if constexpr (OP != O_REPLACE) {
                asm volatile("" : "+v"(a[0]), "+v"(a[1]), "+v"(b[0]), "+v"(b[1]));
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int u = 0; u < 2; ++u)
                st_pol<POL::st>(vio + i0 + (size_t)u * BLOCK, vio + t0, off0 + (unsigned)u * BLOCK * 16u,
                                widen_apply_vec<OP, H>(b[u], a[u]));
        } else {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const size_t i = i0 + (size_t)u * BLOCK;
                if (i < nq) {
                    const u32x2 x = vin[i];
                    u32x4 y = {};
                    if constexpr (OP != O_REPLACE) y = vio[i];
                    vio[i] = widen_apply_vec<OP, H>(y, x);
                }
            }
        }
    }

    const size_t nscalar = head + tail;
    if (nscalar) {
        const size_t body_end = head + nvec * 8;
        for (size_t s = (size_t)blockIdx.x * BLOCK + threadIdx.x; s < nscalar; s += (size_t)gridDim.x * BLOCK) {
            const size_t e = s < head ? s : body_end + (s - head);
            uint32_t y = 0;
            if constexpr (OP != O_REPLACE) y = io[e];
            io[e] = widen_apply<OP>(y, widen_bits<H>(in[e]));
        }
    }
}

// One element at any byte address (ALIGNED: origin % 2 == 0, target % 4 == 0).
template <int OP, class H, bool ALIGNED>
__device__ __forceinline__ void widen_elem(char* t, const char* o)
{
    if constexpr (ALIGNED) {
        uint32_t* tt = reinterpret_cast<uint32_t*>(t);
        uint32_t y = 0;
        if constexpr (OP != O_REPLACE) y = *tt;
        *tt = widen_apply<OP>(y, widen_bits<H>(*reinterpret_cast<const uint16_t*>(o)));
    } else {
        uint16_t x;
        uint32_t y = 0;
        __builtin_memcpy(&x, o, 2);
        if constexpr (OP != O_REPLACE) __builtin_memcpy(&y, t, 4);
        y = widen_apply<OP>(y, widen_bits<H>(x));
        __builtin_memcpy(t, &y, 4);
    }
}

// Operand split of the vector body: it runs when one head h in 0..7 makes both
// origin + 2 h and target + 4 h multiples of 16; any other placement of
// naturally aligned operands is all-scalar (there is no realigning kernel).
__host__ inline void widen_split(const void* in, const void* io, size_t count, size_t& head, size_t& nvec,
                                 size_t& tail)
{
    const uintptr_t a = (uintptr_t)in, b = (uintptr_t)io;
    size_t h = ((16 - (a & 15)) & 15) / 2;
    if ((a & 1) || ((b + 4 * h) & 15)) {
        head = count; nvec = 0; tail = 0;
        return;
    }
    if (h > count) h = count;
    const size_t rest = count - h;
    head = h; nvec = rest / 8; tail = rest - nvec * 8;
}

}  // namespace dev
}  // namespace msx
