// device_op_demo.hip — a device-resident user-defined reduction op: abs-max
// written with the kernel kit, registered with its fused tree form and used in
// MPI_Allreduce on device buffers.
//
//   hipcc --offload-arch=gfx950 -Iinclude examples/device_op_demo.hip \
//         -Lmicrosoft-mpi_amd/lib -lmsmpi_mi355x -o device_op_demo
//   MSX_SIZE=2 MSX_RANK=0 ./device_op_demo &  MSX_SIZE=2 MSX_RANK=1 ./device_op_demo
#include <math.h>
#include <stdio.h>
#include <vector>

#include "msx_device_op.h"

struct AbsMax {
    __device__ float operator()(const float& in, const float& inout) const { return fmaxf(fabsf(in), fabsf(inout)); }
};
// extern "C" int absmax_f32(in, inout, count, datatype, stream, state): enqueues the kit's pairwise
// kernel; absmax_f32_tree(srcs, P, pairmask, nleaves, chain, in_left, out, ...): its fused tree, one
// launch for a collective's whole evaluation
MSX_DEVICE_OP_TREE(absmax_f32, float, AbsMax)

int main(int argc, char** argv)
{
    MPI_Init(&argc, &argv);
    int rank = 0, size = 1;
    MPI_Comm_rank(MPI_COMM_WORLD, &rank);
    MPI_Comm_size(MPI_COMM_WORLD, &size);

    const int n = 1 << 20;
    std::vector<float> h((size_t)n);
    for (int i = 0; i < n; ++i) h[(size_t)i] = (i % 2 ? -1.0f : 1.0f) * (float)((i + rank * 7) % 1000);
    float *x = nullptr, *y = nullptr;
    if (hipMalloc(&x, n * sizeof(float)) != hipSuccess || hipMalloc(&y, n * sizeof(float)) != hipSuccess) return 1;
    if (hipMemcpy(x, h.data(), n * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) return 1;

    MPI_Op op;
    msx_op_create_device_tree(absmax_f32, absmax_f32_tree, /*commute=*/1, /*state=*/NULL, &op);
    MPI_Allreduce(x, y, n, MPI_FLOAT, op, MPI_COMM_WORLD);      // the data never leaves the GPU
    MPI_Op_free(&op);

    if (hipMemcpy(h.data(), y, n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return 1;
    int bad = 0;
    for (int i = 0; i < n; ++i) {
        float want = 0;
        for (int r = 0; r < size; ++r) want = fmaxf(want, (float)((i + r * 7) % 1000));
        if (size == 1) want *= (i % 2 ? -1.0f : 1.0f);          // one rank: its own input, nothing combined
        bad += h[(size_t)i] != want;
    }
    printf("rank %d of %d: abs-max over %d floats, %d wrong\n", rank, size, n, bad);
    (void)hipFree(x);
    (void)hipFree(y);
    MPI_Finalize();
    return bad != 0;
}
