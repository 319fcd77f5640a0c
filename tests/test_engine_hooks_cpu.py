"""CPU: the three kernel test hooks of include/msx.h (msx_reduce_tree_done_dev,
msx_push_dev, msx_copy_segs_dev) reject bad arguments with MPI_ERR_ARG before
they touch a GPU, so every call here returns the same on a host without one.
No call in this file is a valid launch: the pointers are host memory."""
import ctypes

import numpy as np

import msx

C = msx.C
VP, I64 = ctypes.c_void_p, ctypes.c_int64


def _arr(ct, vals):
    return (ct * max(1, len(vals)))(*vals)


def test_tree_hook_rejects_bad_arguments():
    L = msx.lib()
    buf = np.zeros(64, np.uint8)
    a = buf.ctypes.data
    srcs = _arr(VP, [a] * 32)
    ptrs = _arr(VP, [a] * 64)

    def call(srcs=srcs, P=4, pm=0, nl=0, chain=0, out=a, extra=None, nextra=0, counter=None, launches=1,
             flags=None, nflags=0, count=8, dt=C.MPI_INT, op=C.MPI_SUM):
        return L.msx_reduce_tree_done_dev(srcs, P, pm, nl, chain, out, extra, nextra, counter, launches, flags,
                                          nflags, 5, count, dt, op, None)

    E = C.MPI_ERR_ARG
    assert call(srcs=None) == E and call(out=None) == E                # null arrays
    assert call(count=-1) == E                                         # negative size
    assert call(P=3) == E and call(P=32) == E and call(P=0) == E       # trees: a power of two <= 16
    assert call(P=17, chain=1) == E and call(P=0, chain=1) == E        # chains: 1..16
    assert call(P=4, pm=0x10) == E and call(P=4, nl=5) == E and call(P=4, nl=-1) == E
    assert call(nextra=-1) == E and call(nextra=32, extra=ptrs) == E   # nextra outside 0..31
    assert call(nextra=2, extra=None) == E
    assert call(nextra=2, extra=_arr(VP, [a, None])) == E
    assert call(nflags=-1, counter=a) == E and call(nflags=65, counter=a, flags=ptrs) == E   # outside 0..64
    assert call(nflags=1, counter=a, flags=None) == E
    assert call(nflags=1, counter=None, flags=ptrs) == E               # flags need the counter
    assert call(nflags=2, counter=a, flags=_arr(VP, [a, None])) == E
    assert call(counter=a, launches=0) == E and call(counter=a, launches=-3) == E
    # the op / datatype checks of msx_reduce_tree_spec_dev come first
    assert call(op=C.MPI_REPLACE) == C.MPI_ERR_OP and call(dt=C.MPI_BYTE) == C.MPI_ERR_OP
    # nothing to do: valid arguments and count 0 return before any launch
    assert call(count=0, nextra=31, extra=ptrs, counter=a, nflags=64, flags=ptrs) == 0


def test_push_hook_rejects_bad_arguments():
    L = msx.lib()
    buf = np.zeros(64, np.uint8)
    a = buf.ctypes.data
    p40 = _arr(VP, [a] * 40)
    n40 = _arr(I64, [8] * 40)

    def call(src=p40, dst=p40, nb=n40, nseg=2, flags=p40, nflags=1, counter=a, wait=a, err=a):
        return L.msx_push_dev(src, dst, nb, nseg, flags, nflags, 7, counter, wait, err, None)

    E = C.MPI_ERR_ARG
    assert call(nseg=-1) == E and call(nseg=33) == E                   # nseg outside 0..32
    assert call(src=None) == E and call(dst=None) == E and call(nb=None) == E
    assert call(nb=_arr(I64, [8, -1])) == E                            # negative size
    assert call(src=_arr(VP, [a, None])) == E and call(dst=_arr(VP, [None, a])) == E
    assert call(nflags=-1) == E and call(nflags=65) == E               # nflags outside 0..64
    assert call(flags=None) == E and call(flags=_arr(VP, [None])) == E
    assert call(counter=None) == E                                     # segments need the counter
    assert call(wait=None) == E and call(err=None) == E                # the two words the launch names
    assert call(nseg=0, src=None, dst=None, nb=None, counter=None, wait=None) == E


def test_copy_segments_hook_rejects_bad_arguments():
    L = msx.lib()
    buf = np.zeros(64, np.uint8)
    a = buf.ctypes.data
    p3, n3 = _arr(VP, [a] * 3), _arr(I64, [8, 0, 8])
    E = C.MPI_ERR_ARG
    assert L.msx_copy_segs_dev(p3, p3, n3, -1, None) == E
    assert L.msx_copy_segs_dev(None, p3, n3, 3, None) == E
    assert L.msx_copy_segs_dev(p3, None, n3, 3, None) == E
    assert L.msx_copy_segs_dev(p3, p3, None, 3, None) == E
    assert L.msx_copy_segs_dev(p3, p3, _arr(I64, [8, -8, 8]), 3, None) == E
    assert L.msx_copy_segs_dev(_arr(VP, [a, None, None]), p3, n3, 3, None) == E     # null source of 8 bytes
    assert L.msx_copy_segs_dev(p3, _arr(VP, [None, None, a]), n3, 3, None) == E
    # nothing to copy: no segments, or only empty ones with null pointers
    assert L.msx_copy_segs_dev(None, None, None, 0, None) == 0


def test_schedule_tree_admits_what_sixteen_leaves_hold():
    """The tree kernels take 16 leaves (kMaxLeaves): the fold trees -- a rank
    or a folded pair per leaf -- reach p = 31, the binomial tree and the
    pairwise chain -- a leaf / a source per rank -- p = 16."""
    L = msx.lib()
    L.msx_schedule_tree.argtypes = [ctypes.c_int] * 3 + [VP] * 4
    src = (ctypes.c_int * 32)()
    P, pm, ch = ctypes.c_int(), ctypes.c_uint(), ctypes.c_int()

    def call(which, p, n):
        return L.msx_schedule_tree(which, p, n, src, ctypes.byref(P), ctypes.byref(pm), ctypes.byref(ch))

    for which in (0, 1, 3):
        assert call(which, 31, 15) == 0 and P.value == 16 and bin(pm.value).count("1") == 15 and \
            sorted(list(src)) == [-1] + list(range(31))          # every rank once; one leaf is unpaired
        assert call(which, 32, 0) == C.MPI_ERR_ARG
    for which in (2, 4):
        assert call(which, 16, 15) == 0 and P.value == 16
        assert call(which, 17, 0) == C.MPI_ERR_ARG
    assert call(0, 8, 8) == C.MPI_ERR_ARG and call(0, 8, -1) == C.MPI_ERR_ARG and call(5, 8, 0) == C.MPI_ERR_ARG
