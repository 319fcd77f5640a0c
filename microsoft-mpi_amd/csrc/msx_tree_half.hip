// msx_tree_half.hip — k_tree launchers for the 16-bit floats (MSX_FLOAT16,
// MSX_BFLOAT16) under MAX, MIN, SUM and PROD, see msx_tree_impl.h.  Every
// combine inside the fused tree goes through Fn<OP>::apply / apply_vec on the
// 16-bit values, so each node's result is rounded before the next one reads it.
#include "msx_tree_impl.h"

namespace msx {
namespace {

template <int OP>
hipError_t tree_half(Kind k, const TreeArgs& a, int ns, void* out, size_t n, hipStream_t s)
{
    if (k == K_F16) return run_tree_auto<OP, f16, f16>(a, ns, out, n, s);
    if (k == K_BF16) return run_tree_auto<OP, bf16, bf16>(a, ns, out, n, s);
    return hipErrorInvalidValue;
}

}  // namespace

hipError_t tree_dispatch_half(int opidx, Kind k, const dev::TreeArgs& a, int ns, void* out, size_t n,
                              hipStream_t s)
{
    switch (opidx) {
    case O_SUM:  return tree_half<O_SUM>(k, a, ns, out, n, s);
    case O_PROD: return tree_half<O_PROD>(k, a, ns, out, n, s);
    case O_MAX:  return tree_half<O_MAX>(k, a, ns, out, n, s);
    case O_MIN:  return tree_half<O_MIN>(k, a, ns, out, n, s);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace msx
