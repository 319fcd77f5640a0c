// devop_ops.hip — device user ops for the tests of msx_op_create_device,
// written with the kernel kit (include/msx_device_op.h) against include/ alone.
//
// Every launcher counts its calls and the elements it was asked to combine, and
// records whether both operands were device memory (devop_stats).  `state`, when
// not NULL, points to a uint32_t salt that is added to every result, so a lost
// state shows in the data.
#include <atomic>
#include <stdint.h>

#include "msx_device_op.h"

namespace {

std::atomic<int64_t> g_calls{0}, g_count{0};
std::atomic<int> g_on_device{1};
std::atomic<int> g_stride2_n{0};

void note(const void* in, const void* inout, int64_t count)
{
    g_calls.fetch_add(1);
    g_count.fetch_add(count);
    if (msx_operands_on_device(in, inout) != 1) g_on_device.store(0);
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

struct AbsMax {
    __device__ float operator()(const float& in, const float& inout) const { return fmaxf(fabsf(in), fabsf(inout)); }
};

struct AddF32 {
    __device__ float operator()(const float& in, const float& inout) const { return in + inout; }
};

// the uint32_t at typed offset 8 * i of each operand, i < n
__global__ __launch_bounds__(256) void k_stride2(const uint32_t* __restrict__ in, uint32_t* __restrict__ io, size_t n,
                                                 uint32_t salt)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        io[2 * i] = 3u * in[2 * i] - io[2 * i] + salt;
}

}  // namespace

#define DEVOP_KIT(name, T, F)                                                                             \
    MSX_DEVICE_OP(name##_kit, T, F)                                                                       \
    extern "C" int name(const void* in, void* inout, int64_t count, MPI_Datatype dt, void* stream, void* state) \
    {                                                                                                     \
        note(in, inout, count);                                                                           \
        return name##_kit(in, inout, count, dt, stream, state);                                           \
    }

DEVOP_KIT(devop_nc_u32, uint32_t, Nc<uint32_t>)
DEVOP_KIT(devop_nc_u8, uint8_t, Nc<uint8_t>)
DEVOP_KIT(devop_nc_u16, uint16_t, Nc<uint16_t>)
DEVOP_KIT(devop_nc_u64, uint64_t, Nc<uint64_t>)
DEVOP_KIT(devop_nc_u64x2, U64x2, NcU64x2)
DEVOP_KIT(devop_nc_u32x3, U32x3, NcU32x3)
DEVOP_KIT(devop_absmax_f32, float, AbsMax)
// the bandwidth probe's functor (scripts/device_op_probe.py): the bare macro,
// no bookkeeping on the enqueue path
MSX_DEVICE_OP(devop_add_f32, float, AddF32)

// devop_nc_u32's host twin (MPI_Op_create)
extern "C" void devop_nc_u32_host(void* in, void* inout, int* len, MPI_Datatype*)
{
    const uint32_t* a = static_cast<const uint32_t*>(in);
    uint32_t* b = static_cast<uint32_t*>(inout);
    for (int i = 0; i < *len; ++i) b[i] = 3u * a[i] - b[i];
}

// MPI_Type_vector(n, 1, 2, MPI_UNSIGNED) passed with count 1: a hand-written
// launcher, not the kit.  n comes from devop_set_stride2_n (a device function
// must not call MPI to ask the datatype).
extern "C" void devop_set_stride2_n(int n) { g_stride2_n.store(n); }

extern "C" int devop_stride2_u32(const void* in, void* inout, int64_t count, MPI_Datatype, void* stream, void* state)
{
    note(in, inout, count);
    const size_t n = (size_t)g_stride2_n.load();
    if (count != 1) return MPI_ERR_COUNT;
    if (n == 0) return MPI_SUCCESS;
    size_t grid = (n + 255) / 256;
    if (grid > 65536) grid = 65536;
    hipLaunchKernelGGL(k_stride2, dim3((unsigned)grid), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint32_t*>(in), static_cast<uint32_t*>(inout), n, salt_of(state));
    return hipGetLastError() == hipSuccess ? MPI_SUCCESS : MPI_ERR_OTHER;
}

extern "C" void devop_stride2_u32_host(void* in, void* inout, int* len, MPI_Datatype*)
{
    const uint32_t* a = static_cast<const uint32_t*>(in);
    uint32_t* b = static_cast<uint32_t*>(inout);
    const int n = *len == 1 ? g_stride2_n.load() : 0;
    for (int i = 0; i < n; ++i) b[2 * i] = 3u * a[2 * i] - b[2 * i];
}

// returns MPI_ERR_ARG and launches nothing
extern "C" int devop_fail(const void*, void*, int64_t, MPI_Datatype, void*, void*) { return MPI_ERR_ARG; }

// the kit with a forced geometry (0 by size, 1 cached form, 2 DRAM form);
// returns the hipError_t
extern "C" int devop_kit_u32(const void* in, void* inout, int64_t count, int geometry, void* stream)
{
    return (int)msx_kit::combine(static_cast<const uint32_t*>(in), static_cast<uint32_t*>(inout), count,
                                 Nc<uint32_t>(nullptr), static_cast<hipStream_t>(stream), geometry);
}

// out = {calls, sum of count, 1 when both operands were device memory on every call}
extern "C" void devop_stats(int64_t out[3], int reset)
{
    out[0] = g_calls.load();
    out[1] = g_count.load();
    out[2] = g_on_device.load();
    if (reset) {
        g_calls.store(0);
        g_count.store(0);
        g_on_device.store(1);
    }
}
