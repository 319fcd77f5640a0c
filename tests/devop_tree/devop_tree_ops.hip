// devop_tree_ops.hip — device user ops with a fused tree function, for the
// tests of msx_op_create_device_tree, written with the kernel kit
// (include/msx_device_op.h) against include/ alone.
//
// Every function counts its calls and the elements it was asked to evaluate,
// the pairwise and the tree functions separately, and records whether every
// pointer it was handed was device memory (devop_tree_stats).  `state`, when
// not NULL, points to a uint32_t salt that is added at every combine, so a
// lost state shows in the data.
#include <atomic>
#include <stdint.h>

#include "msx_device_op.h"

namespace {

std::atomic<int64_t> g_pair_calls{0}, g_pair_count{0}, g_tree_calls{0}, g_tree_count{0}, g_declined{0};
std::atomic<int> g_on_device{1};

void note_pair(const void* in, const void* inout, int64_t count)
{
    g_pair_calls.fetch_add(1);
    g_pair_count.fetch_add(count);
    if (msx_operands_on_device(in, inout) != 1) g_on_device.store(0);
}

// the slots a tree function may read: a chain's P, the present leaves and the
// pairs the mask names
void note_tree(const void* const* srcs, int P, unsigned pairmask, int nleaves, int chain, const void* out,
               int64_t count)
{
    g_tree_calls.fetch_add(1);
    g_tree_count.fetch_add(count);
    const int nl = nleaves ? nleaves : P;
    for (int k = 0; k < (chain ? P : nl); ++k) {
        const void* a = srcs[chain ? k : 2 * k];
        const void* b = (!chain && ((pairmask >> k) & 1u)) ? srcs[2 * k + 1] : a;
        if (msx_operands_on_device(a, b) != 1) g_on_device.store(0);
    }
    if (msx_operands_on_device(out, out) != 1) g_on_device.store(0);
}

uint32_t salt_of(void* state) { return state ? *static_cast<const uint32_t*>(state) : 0u; }

// in (op) inout = 3 * in - inout (+ salt), wrapping: neither commutative nor
// associative, so a swapped role or another association changes bits
template <class T>
struct Nc {
    T salt;
    explicit Nc(void* state) : salt((T)salt_of(state)) {}
    __device__ T operator()(const T& in, const T& inout) const { return (T)((T)3 * in - inout + salt); }
};

struct U64x2 { uint64_t a, b; };
struct NcU64x2 {
    uint64_t salt;
    explicit NcU64x2(void* state) : salt(salt_of(state)) {}
    __device__ U64x2 operator()(const U64x2& in, const U64x2& io) const
    {
        return U64x2{3 * in.a - io.a + salt, 3 * in.b - io.b + salt};
    }
};

struct U32x3 { uint32_t a, b, c; };
struct NcU32x3 {
    uint32_t salt;
    explicit NcU32x3(void* state) : salt(salt_of(state)) {}
    __device__ U32x3 operator()(const U32x3& in, const U32x3& io) const
    {
        return U32x3{3 * in.a - io.a + salt, 3 * in.b - io.b + salt, 3 * in.c - io.c + salt};
    }
};
static_assert(sizeof(U64x2) == 16 && sizeof(U32x3) == 12, "record sizes");

struct AddF32 {
    __device__ float operator()(const float& in, const float& inout) const { return in + inout; }
};

}  // namespace

// `name` (pairwise) and `name_tree`, both counted, over the kit's pair
#define DEVOP_TREE_KIT(name, T, F)                                                                          \
    MSX_DEVICE_OP_TREE(name##_kit, T, F)                                                                    \
    extern "C" int name(const void* in, void* inout, int64_t count, MPI_Datatype dt, void* stream, void* state) \
    {                                                                                                       \
        note_pair(in, inout, count);                                                                        \
        return name##_kit(in, inout, count, dt, stream, state);                                             \
    }                                                                                                       \
    extern "C" int name##_tree(const void* const* srcs, int P, unsigned pairmask, int nleaves, int chain,   \
                               int in_left, void* out, int64_t count, MPI_Datatype dt, void* stream,        \
                               void* state)                                                                 \
    {                                                                                                       \
        note_tree(srcs, P, pairmask, nleaves, chain, out, count);                                           \
        return name##_kit_tree(srcs, P, pairmask, nleaves, chain, in_left, out, count, dt, stream, state);  \
    }

DEVOP_TREE_KIT(devop_tree_nc_u32, uint32_t, Nc<uint32_t>)
DEVOP_TREE_KIT(devop_tree_nc_u8, uint8_t, Nc<uint8_t>)
DEVOP_TREE_KIT(devop_tree_nc_u16, uint16_t, Nc<uint16_t>)
DEVOP_TREE_KIT(devop_tree_nc_u64, uint64_t, Nc<uint64_t>)
DEVOP_TREE_KIT(devop_tree_nc_u64x2, U64x2, NcU64x2)
DEVOP_TREE_KIT(devop_tree_nc_u32x3, U32x3, NcU32x3)
// the probe's functor (scripts/device_op_tree_probe.py): the bare macro, no
// bookkeeping on the enqueue path
MSX_DEVICE_OP_TREE(devop_tree_add_f32, float, AddF32)

// devop_tree_nc_u32's host twin (MPI_Op_create)
extern "C" void devop_tree_nc_u32_host(void* in, void* inout, int* len, MPI_Datatype*)
{
    const uint32_t* a = static_cast<const uint32_t*>(in);
    uint32_t* b = static_cast<uint32_t*>(inout);
    for (int i = 0; i < *len; ++i) b[i] = 3u * a[i] - b[i];
}

// always declines and enqueues nothing: registered beside devop_tree_nc_u32,
// the library must run the pairwise calls
extern "C" int devop_tree_decline(const void* const*, int, unsigned, int, int, int, void*, int64_t, MPI_Datatype,
                                  void*, void*)
{
    g_declined.fetch_add(1);
    return MSX_TREE_DECLINED;
}

// returns MPI_ERR_ARG and enqueues nothing
extern "C" int devop_tree_fail(const void* const*, int, unsigned, int, int, int, void*, int64_t, MPI_Datatype, void*,
                               void*)
{
    g_tree_calls.fetch_add(1);
    return MPI_ERR_ARG;
}

// the kit with a forced geometry (0 by size, 1 cached form, 2 DRAM form);
// returns the hipError_t
extern "C" int devop_tree_kit_u32(const void* const* srcs, int P, unsigned pairmask, int nleaves, int chain,
                                  int in_left, void* out, int64_t count, int geometry, void* stream)
{
    return (int)msx_kit::tree<uint32_t>(srcs, P, pairmask, nleaves, chain, in_left, out, count,
                                        Nc<uint32_t>(nullptr), static_cast<hipStream_t>(stream), geometry);
}

// seven pairwise launches over p = 8 blocks in the order of a full 8-leaf tree
// with in_left = 0 (the sequence the fused call replaces; the probe's yardstick):
// x[0] ends as the tree's value, the other blocks are overwritten
extern "C" int devop_tree_add_f32_pairwise8(void* const* x, int64_t count, void* stream)
{
    hipStream_t s = static_cast<hipStream_t>(stream);
    for (int w = 1; w < 8; w *= 2)
        for (int k = 0; k + w < 8; k += 2 * w) {
            const hipError_t e = msx_kit::combine(static_cast<const float*>(x[k + w]), static_cast<float*>(x[k]), count,
                                                  AddF32{}, s);
            if (e != hipSuccess) return (int)e;
        }
    return 0;
}

// out = {pairwise calls, pairwise elements, tree calls, tree elements,
//        1 when every pointer of every call was device memory, declined calls}
extern "C" void devop_tree_stats(int64_t out[6], int reset)
{
    out[0] = g_pair_calls.load();
    out[1] = g_pair_count.load();
    out[2] = g_tree_calls.load();
    out[3] = g_tree_count.load();
    out[4] = g_on_device.load();
    out[5] = g_declined.load();
    if (reset) {
        g_pair_calls.store(0);
        g_pair_count.store(0);
        g_tree_calls.store(0);
        g_tree_count.store(0);
        g_declined.store(0);
        g_on_device.store(1);
    }
}
