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
 *
 * msx_kit::tree<T, F> and MSX_DEVICE_OP_TREE (below) add the fused form: one
 * launch that evaluates a collective's whole reduction tree of the same
 * functor, for msx_op_create_device_tree.
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

/* ---- the fused p-way tree (msx_op_create_device_tree) ----------------------
 *
 * msx_kit::tree<T, F>(srcs, P, pairmask, nleaves, chain, in_left, out, count,
 *                     f, stream) enqueues ONE launch that evaluates a whole
 * reduction tree of the pairwise functor per element: every source is read
 * once and `out` written once (p + 1 element sizes per result element against
 * the 3 (p - 1) of p - 1 combine launches).  The slot layout and the value are
 * those of MSX_Device_tree_function (msx.h); it restates the library's builtin
 * tree kernel for any functor:
 *
 *   Fixed form.  Full trees of 2, 4 or 8 leaves: the leaf count is a template
 *     parameter, the fold pattern (pairmask) a run-time value.  Every source
 *     vector of a lane is loaded unconditionally before the first combine; an
 *     unpaired leaf loads its own vector again as its "pair" (the same address
 *     in the same wave: L2, not HBM) and the pattern picks results with
 *     wave-uniform selects.  A tree without pairs loads the leaves only.
 *   Generic form.  Everything else (absent leaves, chains, 16 leaves): loads
 *     interleaved with the combines under wave-uniform leaf tests.
 *   Roles.  in_left is a wave-uniform run-time selection of the functor's
 *     operands, not a second set of kernels.
 *   Vector path.  sizeof(T) 1, 2, 4, 8 or 16 and every source and `out` at one
 *     offset from 16-byte alignment; head and tail elements run as scalars in
 *     the same launch.  Otherwise one T per lane, grid-stride.
 *   Geometry.  Up to 256 MiB of source bytes per launch: 256-lane workgroups
 *     over XCD-contiguous tiles with plain loads.  Above: one-wave workgroups
 *     in dispatch order with non-temporal loads.
 *
 * Sources are never written.  `out` may be one of the sources or disjoint from
 * all of them: a lane reads element i of every source before it writes
 * element i of `out`, and no other lane touches element i. */
namespace detail {

constexpr int kTreeMaxLeaves = 16;
constexpr size_t kTreeNtMin = (size_t)256 << 20;   /* source bytes of one launch */
constexpr unsigned kTreeGridCap = 4096;            /* generic form, 256 lanes: grid-stride beyond */
constexpr unsigned kTreeTileGridCap = 1u << 20;    /* one tile per workgroup up to here */

struct TreeArgs {
    const void* s[2 * kTreeMaxLeaves];
    int P;
    int nleaves;        /* leaves present, 1..P (trees) */
    unsigned pairmask;
    int chain;
    int in_left;
};

template <bool NT>
__device__ __forceinline__ u32x4 ld(const u32x4* p)
{
    if constexpr (NT) return __builtin_nontemporal_load(p);
    else return *p;
}

/* One combine of a left and a right value.  in_left == 0: the right value is
 * the functor's `in` and the left one its `inout`; in_left == 1: the reverse. */
template <class T, class F>
struct TreeFn {
    F f;
    bool il;
    __device__ __forceinline__ u32x4 vec(u32x4 l, u32x4 r) const
    {
        const u32x4 in = il ? l : r, io = il ? r : l;
        return apply_vec<T, F>(in, io, f);
    }
    __device__ __forceinline__ T elem(const T& l, const T& r) const
    {
        const T in = il ? l : r, io = il ? r : l;
        return f(in, io);
    }
};

/* The NL-leaf full tree over v[k] (leaf k) and, MASKED, w[k] (its fold pair
 * where bit k of pm is set; a copy of the leaf elsewhere). */
template <class V, int NL, bool MASKED, class AP>
__device__ __forceinline__ V tree_fixed_reduce(V* v, const V* w, unsigned pm, AP ap)
{
    if constexpr (MASKED) {
#pragma unroll
        for (int k = 0; k < NL; ++k) {
            const V fk = ap(v[k], w[k]);
            if ((pm >> k) & 1u) v[k] = fk;
        }
    }
#pragma unroll
    for (int d = 1; d < NL; d *= 2) {
#pragma unroll
        for (int k = 0; k + d < NL; k += 2 * d) v[k] = ap(v[k], v[k + d]);
    }
    return v[0];
}

/* Any tree or chain, loads taken as the evaluation consumes them.  Leaves >=
 * nleaves are absent: a node whose right subtree is empty passes its left
 * value up unchanged. */
template <class V, class LD, class AP>
__device__ __forceinline__ V tree_eval(const TreeArgs& a, LD load, AP ap)
{
    if (a.chain) {
        V x[kTreeMaxLeaves];
#pragma unroll
        for (int k = 0; k < kTreeMaxLeaves; ++k)
            if (k < a.P) x[k] = load(k);
        V v = x[0];
#pragma unroll
        for (int k = 1; k < kTreeMaxLeaves; ++k)
            if (k < a.P) v = ap(v, x[k]);
        return v;
    }
    V v[kTreeMaxLeaves];
#pragma unroll
    for (int k = 0; k < kTreeMaxLeaves; ++k) {
        if (k < a.nleaves) {
            v[k] = load(2 * k);
            if ((a.pairmask >> k) & 1u) v[k] = ap(v[k], load(2 * k + 1));
        }
    }
#pragma unroll
    for (int w = 1; w < kTreeMaxLeaves; w *= 2) {
#pragma unroll
        for (int k = 0; k + w < kTreeMaxLeaves; k += 2 * w)
            if (k + w < a.nleaves) v[k] = ap(v[k], v[k + w]);
    }
    return v[0];
}

/* Scalar element s of the head + tail elements round a vector body -> element index */
__device__ __forceinline__ size_t tree_scalar_index(size_t s, size_t head, size_t nvec, size_t epv)
{
    return s < head ? s : head + nvec * epv + (s - head);
}

/* Fixed form.  Vector body: elements [head, head + nvec * EPV); DRAM: dispatch
 * order and non-temporal loads (one-wave workgroups), else XCD-contiguous. */
template <class T, class F, int NL, int BLOCK, bool DRAM, bool MASKED>
__global__ __launch_bounds__(BLOCK) void k_tree_fixed(TreeArgs a, T* out, size_t head, size_t nvec, size_t tail, F f)
{
    constexpr size_t EPV = 16 / sizeof(T);
    const TreeFn<T, F> fn{f, a.in_left != 0};
    const unsigned pm = a.pairmask;
    const u32x4* src[NL];
    const u32x4* src2[MASKED ? NL : 1];
#pragma unroll
    for (int k = 0; k < NL; ++k) {
        src[k] = reinterpret_cast<const u32x4*>(static_cast<const T*>(a.s[2 * k]) + head);
        if constexpr (MASKED) src2[k] = reinterpret_cast<const u32x4*>(static_cast<const T*>(a.s[2 * k + 1]) + head);
    }
    u32x4* vout = reinterpret_cast<u32x4*>(out + head);
    const size_t bid = DRAM ? (size_t)blockIdx.x : (size_t)xcd_tile(blockIdx.x, gridDim.x);
    for (size_t t0 = bid * BLOCK; t0 < nvec; t0 += (size_t)gridDim.x * BLOCK) {
        const size_t i = t0 + threadIdx.x;
        if (i < nvec) {
            u32x4 v[NL], w[MASKED ? NL : 1];
#pragma unroll
            for (int k = 0; k < NL; ++k) {
                v[k] = ld<DRAM>(src[k] + i);
                if constexpr (MASKED) w[k] = ld<DRAM>(src2[k] + i);
            }
            __builtin_amdgcn_sched_barrier(0);      /* every load issued before the first combine */
            vout[i] = tree_fixed_reduce<u32x4, NL, MASKED>(v, w, pm,
                                                           [&](u32x4 l, u32x4 r) { return fn.vec(l, r); });
        }
    }
    const size_t nscalar = head + tail;
    for (size_t s = (size_t)blockIdx.x * BLOCK + threadIdx.x; s < nscalar; s += (size_t)gridDim.x * BLOCK) {
        const size_t e = tree_scalar_index(s, head, nvec, EPV);
        T v[NL], w[MASKED ? NL : 1];
#pragma unroll
        for (int k = 0; k < NL; ++k) {
            v[k] = static_cast<const T*>(a.s[2 * k])[e];
            if constexpr (MASKED) w[k] = static_cast<const T*>(a.s[2 * k + 1])[e];
        }
        out[e] = tree_fixed_reduce<T, NL, MASKED>(v, w, pm, [&](const T& l, const T& r) { return fn.elem(l, r); });
    }
}

/* Generic form, and with nvec == 0 the all-scalar path (head = count). */
template <class T, class F, int BLOCK, bool DRAM>
__global__ __launch_bounds__(BLOCK) void k_tree_any(TreeArgs a, T* out, size_t head, size_t nvec, size_t tail, F f)
{
    const TreeFn<T, F> fn{f, a.in_left != 0};
    const size_t stride = (size_t)gridDim.x * BLOCK;
    size_t epv = 1;
    if constexpr (vector_size<T>()) {
        epv = 16 / sizeof(T);
        u32x4* vout = reinterpret_cast<u32x4*>(out + head);
        const size_t bid = DRAM ? (size_t)blockIdx.x : (size_t)xcd_tile(blockIdx.x, gridDim.x);
        for (size_t i = bid * BLOCK + threadIdx.x; i < nvec; i += stride) {
            auto load = [&](int k) { return ld<DRAM>(reinterpret_cast<const u32x4*>(static_cast<const T*>(a.s[k]) + head) + i); };
            vout[i] = tree_eval<u32x4>(a, load, [&](u32x4 l, u32x4 r) { return fn.vec(l, r); });
        }
    }
    const size_t nscalar = head + tail;
    for (size_t s = (size_t)blockIdx.x * BLOCK + threadIdx.x; s < nscalar; s += stride) {
        const size_t e = tree_scalar_index(s, head, nvec, epv);
        auto load = [&](int k) { return static_cast<const T*>(a.s[k])[e]; };
        out[e] = tree_eval<T>(a, load, [&](const T& l, const T& r) { return fn.elem(l, r); });
    }
}

inline unsigned tree_grid(size_t nvec, size_t nscalar, size_t block, unsigned cap)
{
    size_t grid = (nvec + block - 1) / block;
    const size_t sc = (nscalar + block - 1) / block;
    if (grid < sc) grid = sc;
    if (grid > cap) grid = cap;          /* every loop strides by the grid */
    return grid ? (unsigned)grid : 1u;
}

template <class T, class F, int NL, bool MASKED>
void launch_tree_fixed(const TreeArgs& a, T* out, size_t head, size_t nvec, size_t tail, F f, bool dram,
                       hipStream_t stream)
{
    if (dram) {
        const unsigned grid = tree_grid(nvec, head + tail, 64, kTreeTileGridCap);
        hipLaunchKernelGGL((k_tree_fixed<T, F, NL, 64, true, MASKED>), dim3(grid), dim3(64), 0, stream, a, out, head,
                           nvec, tail, f);
    } else {
        const unsigned grid = tree_grid(nvec, head + tail, 256, kTreeTileGridCap);
        hipLaunchKernelGGL((k_tree_fixed<T, F, NL, 256, false, MASKED>), dim3(grid), dim3(256), 0, stream, a, out,
                           head, nvec, tail, f);
    }
}

template <class T, class F>
void launch_tree_any(const TreeArgs& a, T* out, size_t head, size_t nvec, size_t tail, F f, bool dram,
                     hipStream_t stream)
{
    if (dram) {
        const unsigned grid = tree_grid(nvec, head + tail, 64, kTreeTileGridCap);
        hipLaunchKernelGGL((k_tree_any<T, F, 64, true>), dim3(grid), dim3(64), 0, stream, a, out, head, nvec, tail, f);
    } else {
        const unsigned grid = tree_grid(nvec, head + tail, 256, kTreeGridCap);
        hipLaunchKernelGGL((k_tree_any<T, F, 256, false>), dim3(grid), dim3(256), 0, stream, a, out, head, nvec, tail,
                           f);
    }
}

}  // namespace detail

/* geometry: 0 by size, 1 the cached form (256-lane workgroups, plain loads),
 * 2 the DRAM form (one-wave workgroups, non-temporal loads) at any size. */
template <class T, class F>
hipError_t tree(const void* const* srcs, int P, unsigned pairmask, int nleaves, int chain, int in_left, void* out,
                int64_t count, F f, hipStream_t stream, int geometry = 0)
{
    using namespace detail;
    if (count < 0 || geometry < 0 || geometry > 2 || !srcs || !out || (in_left != 0 && in_left != 1))
        return hipErrorInvalidValue;
    if (chain) {
        if (P < 2 || P > kTreeMaxLeaves || pairmask != 0 || nleaves != 0) return hipErrorInvalidValue;
    } else {
        if (P < 1 || P > kTreeMaxLeaves || (P & (P - 1)) != 0 || nleaves < 0 || nleaves > P) return hipErrorInvalidValue;
        if ((pairmask >> (nleaves ? nleaves : P)) != 0) return hipErrorInvalidValue;
    }
    if (count == 0) return hipSuccess;
    TreeArgs a{};
    a.P = P;
    a.chain = chain ? 1 : 0;
    a.in_left = in_left;
    a.pairmask = chain ? 0u : pairmask;
    a.nleaves = chain ? 0 : (nleaves ? nleaves : P);
    /* slots that are read: a chain's P, a tree's present leaves and their pairs.
     * An unpaired slot names its own leaf and an absent one leaf 0, so that no
     * slot the kernels could load from is left unset. */
    const uintptr_t off = (uintptr_t)out & 15;
    bool same_off = true;
    size_t nread = 0;
    auto take = [&](int slot, const void* p) {
        a.s[slot] = p;
        same_off = same_off && ((uintptr_t)p & 15) == off;
        ++nread;
    };
    if (chain) {
        for (int k = 0; k < P; ++k) {
            if (!srcs[k]) return hipErrorInvalidValue;
            take(k, srcs[k]);
        }
    } else {
        for (int k = 0; k < a.nleaves; ++k) {
            if (!srcs[2 * k]) return hipErrorInvalidValue;
            take(2 * k, srcs[2 * k]);
            if ((pairmask >> k) & 1u) {
                if (!srcs[2 * k + 1]) return hipErrorInvalidValue;
                take(2 * k + 1, srcs[2 * k + 1]);
            } else {
                a.s[2 * k + 1] = srcs[2 * k];
            }
        }
        for (int k = a.nleaves; k < P; ++k) a.s[2 * k] = a.s[2 * k + 1] = a.s[0];
    }
    const size_t n = (size_t)count;
    const bool dram = geometry == 2 || (geometry == 0 && n * sizeof(T) * nread > kTreeNtMin);
    T* o = static_cast<T*>(out);
    if constexpr (vector_size<T>()) {
        constexpr size_t ES = sizeof(T);
        if (same_off && (off % ES) == 0 && !(ES == 16 && off)) {
            size_t head = ((16 - off) & 15) / ES;
            if (head > n) head = n;
            const size_t epv = 16 / ES;
            const size_t nvec = (n - head) / epv, tail = (n - head) - nvec * epv;
            const bool full = !chain && a.nleaves == P;
            const bool masked = a.pairmask != 0;
            if (full && (P == 2 || P == 4 || P == 8)) {
                if (P == 2 && masked) launch_tree_fixed<T, F, 2, true>(a, o, head, nvec, tail, f, dram, stream);
                else if (P == 2) launch_tree_fixed<T, F, 2, false>(a, o, head, nvec, tail, f, dram, stream);
                else if (P == 4 && masked) launch_tree_fixed<T, F, 4, true>(a, o, head, nvec, tail, f, dram, stream);
                else if (P == 4) launch_tree_fixed<T, F, 4, false>(a, o, head, nvec, tail, f, dram, stream);
                else if (masked) launch_tree_fixed<T, F, 8, true>(a, o, head, nvec, tail, f, dram, stream);
                else launch_tree_fixed<T, F, 8, false>(a, o, head, nvec, tail, f, dram, stream);
            } else {
                launch_tree_any<T, F>(a, o, head, nvec, tail, f, dram, stream);
            }
            return hipGetLastError();
        }
    }
    /* all-scalar: the generic kernel with no vector body */
    launch_tree_any<T, F>(a, o, n, 0, 0, f, dram, stream);
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

/* MSX_DEVICE_OP(name, T, F) plus `extern "C" int name_tree(...)` with the
 * MSX_Device_tree_function shape, which enqueues msx_kit::tree<T, F>; register
 * the two with msx_op_create_device_tree(name, name_tree, commute, state, &op). */
#define MSX_DEVICE_OP_TREE(name, T, F)                                                                  \
    MSX_DEVICE_OP(name, T, F)                                                                           \
    extern "C" int name##_tree(const void* const* srcs, int P, unsigned pairmask, int nleaves, int chain, \
                               int in_left, void* out, int64_t count, MPI_Datatype datatype, void* stream, \
                               void* state)                                                             \
    {                                                                                                   \
        (void)datatype;                                                                                 \
        const hipError_t e = msx_kit::tree<T, F>(srcs, P, pairmask, nleaves, chain, in_left, out, count, \
                                                 msx_kit::detail::make<F>(state),                       \
                                                 static_cast<hipStream_t>(stream));                     \
        return e == hipSuccess ? MPI_SUCCESS : MPI_ERR_OTHER;                                           \
    }

#endif
