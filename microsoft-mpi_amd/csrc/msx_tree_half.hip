// msx_tree_half.hip — k_tree launchers for the 16-bit floats (MSX_FLOAT16,
// MSX_BFLOAT16) under MAX, MIN, SUM and PROD, see msx_tree_impl.h.  Every
// combine inside the fused tree goes through Fn<OP>::apply / apply_vec on the
// 16-bit values, so each node's result is rounded before the next one reads it.
#include "msx_tree_impl.h"

namespace msx {

hipError_t tree_dispatch_half(int opidx, Kind k, const dev::TreeArgs& a, int ns, void* out, size_t n,
                              hipStream_t s)
{
    return for_op(opidx, [&](auto op) {
        return for_kind<decltype(op)::value, C_HALF>(k, [&](auto t) {
            using T = typename decltype(t)::type;
            return run_tree_auto<decltype(op)::value, T, T>(a, ns, out, n, s);
        });
    });
}

}  // namespace msx
