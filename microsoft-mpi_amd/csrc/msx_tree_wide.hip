// msx_tree_wide.hip — k_tree launchers for MSX_SUM_WIDE (msx.h) on the 16-bit
// floats, see msx_tree_impl.h: the same launch forms as every other op
// (run_tree_auto), with the wide tree body of msx_tree_dev.h -- leaves widened
// to fp32 where a node consumes them, every node the fp32 Fn<O_SUM>, the root
// narrowed once.
#include "msx_tree_impl.h"

namespace msx {

hipError_t tree_dispatch_wide(Kind k, const dev::TreeArgs& a, int ns, void* out, size_t n, hipStream_t s)
{
    // the kinds of MPI_SUM's 16-bit floats
    return for_kind<O_SUM, C_HALF>(k, [&](auto t) {
        using T = typename decltype(t)::type;
        // One source and no combine (a chain of one, a tree whose only leaf has no
        // pair): the result is the source's bits, signalling NaNs included.  The
        // per-node kernel copies them (no node runs, so the op does not matter)
        // with the same extra destinations and result-ready count.
        if (a.chain ? a.P == 1 : (a.nleaves == 1 && (a.pairmask & 1u) == 0))
            return tree_dispatch_half(O_SUM, k, a, ns, out, n, s);
        return run_tree_auto<O_SUM_WIDE, T, T>(a, ns, out, n, s);
    });
}

}  // namespace msx
