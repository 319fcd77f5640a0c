/*
 * msx_device_op.h — the kernel kit for device-resident user-defined reduction
 * ops (msx_op_create_device, msx.h).  HIP C++, header-only: compile it with
 * your own `hipcc --offload-arch=gfx950`.  It includes <hip/hip_runtime.h> and
 * msx.h, nothing of the library's sources.
 *
 *   struct AbsMax {
 *       __device__ float operator()(const float& in, const float& inout) const
 *       { return fmaxf(fabsf(in), fabsf(inout)); }
 *   };
 *   MSX_DEVICE_OP(absmax_f32, float, AbsMax)        // extern "C" int absmax_f32(...)
 *   ...
 *   MPI_Op op;
 *   msx_op_create_device(absmax_f32, 1, NULL, &op);
 *   MPI_Allreduce(MPI_IN_PLACE, dev_buf, n, MPI_FLOAT, op, MPI_COMM_WORLD);
 *
 * msx_kit::combine<T, F>(in, inout, count, f, stream) enqueues
 *     inout[i] = f(in[i], inout[i]),  i in [0, count)
 * on `stream` and returns.  `in` is the left operand, as MPI defines a user
 * function.  It restates the streaming form of the library's builtin combine
 *  for any functor:
 *
 *   Vector body.  When sizeof(T) is 1, 2, 4, 8 or 16 each lane moves one
 *     16-byte vector per operand: every load of a tile is issued before the
 *     first use, loads are non-temporal, stores are plain, the elements are
 *     unpacked from the vector in registers and f is applied to each.
 *   Head and tail.  The elements before 16-byte alignment and the ragged end
 *     run as scalars in the same launch.
 *   Geometry by size.  Up to 16 MiB per operand: 256-lane workgroups over
 *     XCD-contiguous tiles.  Above: one-wave workgroups, XCD x owning
 *     interleaved runs of 128 consecutive 1-KiB tiles.
 *   Scalar path.  Operands whose offsets from 16-byte alignment disagree run
 *     all-scalar, and so does a T of any other size (a 12-byte record, say):
 *     one T per lane, grid-stride.  There is NO realigning kernel in the kit;
 *     mutually misaligned operands are correct but slower.
 *
 * Both operands must be aligned for T.  T and F must be trivially copyable;
 * F is passed to the kernel by value.
 */
#ifndef MSX_DEVICE_OP_H_INCLUDED
#define MSX_DEVICE_OP_H_INCLUDED

#include <hip/hip_runtime.h>
#include "msx.h"

namespace msx_kit {
namespace detail {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

/* Both registers are inputs of one (empty) asm statement: their loads are
 * issued back to back and waited for together, and no use of either can be
 * scheduled between them. */
__device__ __forceinline__ void issued_together(u32x4& x, u32x4& y)
{
    asm volatile("" : "+v"(x), "+v"(y));
    __builtin_amdgcn_sched_barrier(0);
}

/* Workgroup b is dispatched to XCD b % 8: XCD x takes one contiguous eighth
 * of the tiles (a bijection for every nb). */
__device__ __forceinline__ unsigned xcd_tile(unsigned b, unsigned nb)
{
    const unsigned q = nb >> 3, r = nb & 7, x = b & 7, j = b >> 3;
    return x * q + (x < r ? x : r) + j;
}

/* XG == 0: XCD-contiguous eighths; XG > 0: XCD x owns interleaved runs of XG
 * consecutive tiles, the remainder below a whole round of 8 * XG tiles in
 * dispatch order. */
template <int XG>
__device__ __forceinline__ size_t combine_tile(unsigned b, unsigned nb)
{
    if constexpr (XG == 0) {
        return xcd_tile(b, nb);
    } else {
        const unsigned full = (nb / (8u * XG)) * (8u * XG);
        if (b >= full) return b;
        const unsigned x = b & 7, j = b >> 3;
        return ((size_t)(j / XG) * 8 + x) * XG + (j % XG);
    }
}

template <class T, class F>
__device__ __forceinline__ u32x4 apply_vec(u32x4 in, u32x4 io, const F& f)
{
    constexpr int N = 16 / (int)sizeof(T);
    T a[N], b[N];
    __builtin_memcpy(a, &in, 16);
    __builtin_memcpy(b, &io, 16);
#pragma unroll
    for (int j = 0; j < N; ++j) b[j] = f(a[j], b[j]);
    u32x4 r;
    __builtin_memcpy(&r, b, 16);
    return r;
}

/* Elements [0, head) and [head + nvec * EPV, head + nvec * EPV + tail) are
 * scalar; the vector body starts at element `head`, 16-byte aligned for both
 * operands.  One tile = BLOCK vectors. */
template <class T, class F, int BLOCK, int XG>
__global__ __launch_bounds__(BLOCK) void k_vec(const T* __restrict__ in, T* __restrict__ io, size_t head,
                                               size_t nvec, size_t tail, F f)
{
    constexpr size_t EPV = 16 / sizeof(T);
    const u32x4* __restrict__ vin = reinterpret_cast<const u32x4*>(in + head);
    u32x4* __restrict__ vio = reinterpret_cast<u32x4*>(io + head);
    const size_t bid = combine_tile<XG>(blockIdx.x, gridDim.x);

    for (size_t t0 = bid * BLOCK; t0 < nvec; t0 += (size_t)gridDim.x * BLOCK) {
        const size_t i = t0 + threadIdx.x;
        if (t0 + BLOCK <= nvec) {
            u32x4 a = __builtin_nontemporal_load(vin + i);
            u32x4 b = __builtin_nontemporal_load(vio + i);
            issued_together(a, b);
            vio[i] = apply_vec<T, F>(a, b, f);
        } else if (i < nvec) {
            u32x4 a = vin[i], b = vio[i];
            issued_together(a, b);
            vio[i] = apply_vec<T, F>(a, b, f);
        }
    }

    const size_t nscalar = head + tail;
    if (nscalar) {
        const size_t body_end = head + nvec * EPV;
        for (size_t s = (size_t)blockIdx.x * BLOCK + threadIdx.x; s < nscalar; s += (size_t)gridDim.x * BLOCK) {
            const size_t e = s < head ? s : body_end + (s - head);
            io[e] = f(in[e], io[e]);
        }
    }
}

/* one T per lane, grid-stride */
template <class T, class F>
__global__ __launch_bounds__(256) void k_scalar(const T* __restrict__ in, T* __restrict__ io, size_t count, F f)
{
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < count; e += (size_t)gridDim.x * 256)
        io[e] = f(in[e], io[e]);
}

template <class T>
constexpr bool vector_size()
{
    return sizeof(T) == 1 || sizeof(T) == 2 || sizeof(T) == 4 || sizeof(T) == 8 || sizeof(T) == 16;
}

/* A functor that has a constructor from void* receives the op's `state`. */
template <class F>
F make(void* state)
{
    if constexpr (__is_constructible(F, void*)) return F(state);
    else return F{};
}

constexpr size_t kDramMin = (size_t)16 << 20;   /* bytes per operand */
constexpr unsigned kGridMax = 0x7fffffffu;

}  // namespace detail

/* geometry: 0 by size, 1 the cached form (256-lane workgroups), 2 the DRAM
 * form (one-wave workgroups, XCD runs) at any size -- for tests and probes. */
template <class T, class F>
hipError_t combine(const T* in, T* inout, int64_t count, F f, hipStream_t stream, int geometry = 0)
{
    using namespace detail;
    if (count < 0 || geometry < 0 || geometry > 2) return hipErrorInvalidValue;
    if (count == 0) return hipSuccess;
    if (!in || !inout) return hipErrorInvalidValue;
    const size_t n = (size_t)count;
    if constexpr (vector_size<T>()) {
        constexpr size_t ES = sizeof(T);
        const uintptr_t a = (uintptr_t)in, b = (uintptr_t)inout;
        if ((a & 15) == (b & 15) && (a % ES) == 0 && !(ES == 16 && (a & 15))) {
            size_t head = ((16 - (a & 15)) & 15) / ES;
            if (head > n) head = n;
            const size_t epv = 16 / ES;
            const size_t nvec = (n - head) / epv, tail = (n - head) - nvec * epv;
            const bool dram = geometry == 2 || (geometry == 0 && nvec * 16 > kDramMin);
            const size_t block = dram ? 64 : 256;
            size_t grid = (nvec + block - 1) / block;
            const size_t sc = (head + tail + block - 1) / block;
            if (grid < sc) grid = sc;
            if (grid > kGridMax) grid = kGridMax;        /* the tile loop strides by the grid */
            if (dram)
                hipLaunchKernelGGL((k_vec<T, F, 64, 128>), dim3((unsigned)grid), dim3(64), 0, stream, in, inout,
                                   head, nvec, tail, f);
            else
                hipLaunchKernelGGL((k_vec<T, F, 256, 0>), dim3((unsigned)grid), dim3(256), 0, stream, in, inout,
                                   head, nvec, tail, f);
            return hipGetLastError();
        }
    }
    size_t grid = (n + 255) / 256;
    if (grid > kGridMax) grid = kGridMax;
    hipLaunchKernelGGL((k_scalar<T, F>), dim3((unsigned)grid), dim3(256), 0, stream, in, inout, n, f);
    return hipGetLastError();
}

}  // namespace msx_kit

/* Defines `extern "C" int name(...)` with the MSX_Device_function shape: it
 * checks nothing about the datatype and enqueues combine<T, F> on the stream
 * it is given.  F is built from `state` when it has a constructor from void*,
 * else value-initialised. */
#define MSX_DEVICE_OP(name, T, F)                                                                       \
    extern "C" int name(const void* in, void* inout, int64_t count, MPI_Datatype datatype, void* stream, \
                        void* state)                                                                    \
    {                                                                                                   \
        (void)datatype;                                                                                 \
        const hipError_t e = msx_kit::combine<T, F>(static_cast<const T*>(in), static_cast<T*>(inout),  \
                                                    count, msx_kit::detail::make<F>(state),             \
                                                    static_cast<hipStream_t>(stream));                  \
        return e == hipSuccess ? MPI_SUCCESS : MPI_ERR_OTHER;                                           \
    }

#endif
