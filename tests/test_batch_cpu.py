"""CPU, no GPU: msx_reduce_local_batch_dev / msx_reduce_local_batch_plan
(include/msx.h): the order of the host-side checks and the plan's figures.

Every check-order case breaks one check and every later one; the class that
comes back names the check that ran first.  The plan is a pure function of its
arguments and never dereferences an address, so it runs on fake device
addresses; the real call is driven only into its checks (and, without a GPU,
to MPI_ERR_OTHER)."""
import ctypes

import pytest

import msx

C = msx.C
vp, i64 = ctypes.c_void_p, ctypes.c_int64

BASE = 0x7F0000000000          # a fake, 16-byte aligned device address
KiB, MiB = 1 << 10, 1 << 20
LIMIT = 16 * MiB               # bytes per operand from which a segment is launched on its own


@pytest.fixture(scope="module")
def L():
    return msx.init(errors_return=True)


def _arrays(ins, ios, counts):
    n = len(counts)
    return (vp * max(n, 1))(*ins), (vp * max(n, 1))(*ios), (i64 * max(n, 1))(*counts)


def _plan(L, ins, ios, counts, dt=None, op=None, nseg=None):
    """(rc, width, launches, batched, single)"""
    a, b, c = _arrays(ins, ios, counts)
    out = [ctypes.c_int(-7) for _ in range(4)]
    rc = L.msx_reduce_local_batch_plan(a, b, c, len(counts) if nseg is None else nseg,
                                       C.MPI_FLOAT if dt is None else dt, C.MPI_SUM if op is None else op,
                                       *[ctypes.byref(o) for o in out])
    return (rc,) + tuple(o.value for o in out)


def _both(L, ins, ios, counts, dt=None, op=None, nseg=None):
    """The class both entry points return for arguments that fail a check."""
    a, b, c = _arrays(ins, ios, counts)
    n = len(counts) if nseg is None else nseg
    dt = C.MPI_FLOAT if dt is None else dt
    op = C.MPI_SUM if op is None else op
    rc = L.msx_reduce_local_batch_dev(a, b, c, n, dt, op, None)
    err = msx.last_error()
    assert rc != 0
    assert _plan(L, ins, ios, counts, dt, op, nseg)[0] == rc
    return rc, err


def _layout(sizes, gap=64, base=BASE, in_base=BASE + (1 << 36)):
    """Disjoint aligned fake segments of `sizes` bytes."""
    ins, ios, o = [], [], 0
    for nb in sizes:
        ins.append(in_base + o)
        ios.append(base + o)
        o += (nb + gap + 15) // 16 * 16
    return ins, ios


@pytest.fixture(scope="module")
def user_op(L):
    UF = ctypes.CFUNCTYPE(None, vp, vp, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int))
    fn = UF(lambda a, b, n, d: None)
    op = ctypes.c_int()
    assert L.MPI_Op_create(fn, 1, ctypes.byref(op)) == 0
    yield op.value
    assert L.MPI_Op_free(ctypes.byref(op)) == 0
    del fn


# ---- the order of the checks -------------------------------------------------------

def test_no_segments_succeeds_with_null_arrays(L):
    assert L.msx_reduce_local_batch_dev(None, None, None, 0, C.MPI_FLOAT, C.MPI_SUM, None) == 0
    out = [ctypes.c_int(-7) for _ in range(4)]
    assert L.msx_reduce_local_batch_plan(None, None, None, 0, C.MPI_FLOAT, C.MPI_SUM,
                                         *[ctypes.byref(o) for o in out]) == 0
    assert out[0].value >= 16 and [o.value for o in out[1:]] == [0, 0, 0]
    # check 1 comes first: not even the op is looked at
    assert L.msx_reduce_local_batch_dev(None, None, None, 0, 0x1234, 0x1234, None) == 0


def test_bad_arrays_come_before_the_op(L, user_op):
    # check 2, with an illegal pair, a negative count, null buffers and aliasing behind it
    ins, ios, counts = [0, BASE], [0, BASE], [-1, 4]
    a, b, c = _arrays(ins, ios, counts)
    for op, dt in ((C.MPI_SUM, C.MPI_BYTE), (user_op, C.MPI_FLOAT), (0x1234, C.MPI_FLOAT)):
        assert L.msx_reduce_local_batch_dev(a, b, c, -1, dt, op, None) == C.MPI_ERR_ARG
        assert L.msx_reduce_local_batch_dev(None, b, c, 2, dt, op, None) == C.MPI_ERR_ARG
        assert L.msx_reduce_local_batch_dev(a, None, c, 2, dt, op, None) == C.MPI_ERR_ARG
        assert L.msx_reduce_local_batch_dev(a, b, None, 2, dt, op, None) == C.MPI_ERR_ARG
        assert _plan(L, ins, ios, counts, dt, op, nseg=-1)[0] == C.MPI_ERR_ARG
    # the plan's own outputs
    assert L.msx_reduce_local_batch_plan(a, b, c, 2, C.MPI_FLOAT, C.MPI_SUM, None, None, None, None) == C.MPI_ERR_ARG


def test_the_op_comes_before_counts_and_buffers(L, user_op):
    # check 3, with a negative count, a null buffer, aliasing and an overlap behind it
    ins, ios, counts = [0, BASE, BASE + 8], [BASE, BASE, BASE], [-1, 4, 4]
    rc, err = _both(L, ins, ios, counts, C.MPI_FLOAT, user_op)
    assert rc == C.MPI_ERR_OP and "builtin ops only" in err
    assert _both(L, ins, ios, counts, C.MPI_BYTE, C.MPI_SUM)[0] == C.MPI_ERR_OP        # illegal pair
    assert _both(L, ins, ios, counts, C.MPI_FLOAT, C.MPI_BXOR)[0] == C.MPI_ERR_OP
    assert _both(L, ins, ios, counts, C.MPI_FLOAT, 0x1234)[0] == C.MPI_ERR_OP          # no op handle
    assert _both(L, ins, ios, counts, C.MPI_FLOAT, C.MPI_REPLACE)[0] == C.MPI_ERR_OP
    assert _both(L, ins, ios, counts, C.MPI_FLOAT, C.MSX_SUM_WIDE)[0] == C.MPI_ERR_OP  # 16-bit floats only


def test_device_user_op_is_refused(L):
    DF = ctypes.CFUNCTYPE(ctypes.c_int, vp, vp, i64, ctypes.c_int, vp, vp)
    fn = DF(lambda *_: 0)
    op = ctypes.c_int()
    assert L.msx_op_create_device(fn, 1, None, ctypes.byref(op)) == 0
    ins, ios = _layout([64, 64])
    rc, err = _both(L, ins, ios, [16, 16], C.MPI_FLOAT, op.value)
    assert rc == C.MPI_ERR_OP and "builtin ops only" in err
    assert L.MPI_Op_free(ctypes.byref(op)) == 0


def test_counts_come_before_buffers(L):
    # check 4: the negative count sits last, behind a null buffer, aliasing and an overlap
    ins, ios, counts = [0, BASE, BASE + 8, BASE + 4096], [BASE, BASE, BASE, BASE + 8192], [4, 4, 4, -1]
    rc, err = _both(L, ins, ios, counts)
    assert rc == C.MPI_ERR_COUNT and "3" in err


def test_null_buffers_come_before_aliasing_and_overlap(L):
    # check 5: the null pointer sits last, behind aliasing and an overlap
    ins, ios, counts = [BASE, BASE + 8, 0], [BASE, BASE, BASE + 8192], [4, 4, 4]
    rc, err = _both(L, ins, ios, counts)
    assert rc == C.MPI_ERR_BUFFER and "null" in err and "2" in err
    ins, ios = [BASE, BASE + 8, BASE + 4096], [BASE, BASE, 0]
    rc, err = _both(L, ins, ios, counts)
    assert rc == C.MPI_ERR_BUFFER and "null" in err


def test_empty_segments_are_skipped_without_looking_at_their_pointers(L):
    # every segment empty: nothing to enqueue, success with or without a GPU
    a, b, c = _arrays([0, 0, BASE], [0, BASE, BASE], [0, 0, 0])
    assert L.msx_reduce_local_batch_dev(a, b, c, 3, C.MPI_FLOAT, C.MPI_SUM, None) == 0
    # null and aliased pointers of empty segments among real ones: not an error
    ins, ios = _layout([64, 64, 64, 64])
    ins[1] = ios[1] = 0
    ins[2] = ios[2] = ios[0]           # an empty segment "inside" segment 0's inout
    assert _plan(L, ins, ios, [16, 0, 0, 16]) == (0, _plan(L, [], [], [])[1], 1, 2, 0)


def test_aliasing_and_overlap(L):
    ins, ios = _layout([256, 256, 256, 256])
    counts = [64, 64, 64, 64]
    assert _plan(L, ins, ios, counts)[0] == 0
    # in[i] == inout[i]
    bad = list(ins)
    bad[2] = ios[2]
    rc, err = _both(L, bad, ios, counts)
    assert rc == C.MPI_ERR_BUFFER and "aliases" in err and "2" in err
    # partial overlap of in[i] and inout[i], from either side
    for d in (-252, -4, 4, 252):
        bad = list(ins)
        bad[1] = ios[1] + d
        rc, err = _both(L, bad, ios, counts)
        assert rc == C.MPI_ERR_BUFFER and "segment 1" in err, (d, err)
    # one byte short of touching: accepted
    bad = list(ins)
    bad[1] = ios[1] + 256
    ios2 = list(ios)
    ios2[2] = ios[2] + 4096            # keep segment 2's inout clear of in[1]
    assert _plan(L, bad, ios2, counts)[0] == 0
    # an inout range overlapping another segment's in: both indices are named
    bad = list(ins)
    bad[3] = ios[0] + 128
    rc, err = _both(L, bad, ios, counts)
    assert rc == C.MPI_ERR_BUFFER and "segment 0" in err and "segment 3" in err, err
    # two inout ranges overlapping (the last segment lands on the first)
    bad = list(ios)
    bad[3] = ios[0] + 252
    rc, err = _both(L, ins, bad, counts)
    assert rc == C.MPI_ERR_BUFFER and "segment 0" in err and "segment 3" in err, err
    # an inout range that contains another one
    rc, err = _both(L, [ins[0], ins[1]], [BASE, BASE + 64], [64, 4])
    assert rc == C.MPI_ERR_BUFFER and "segment 0" in err and "segment 1" in err, err


def test_shared_and_overlapping_in_ranges_are_accepted(L):
    _, ios = _layout([256] * 5)
    src = BASE + (1 << 36)
    ins = [src, src, src + 4, src + 128, src]
    rc, width, launches, batched, single = _plan(L, ins, ios, [64] * 5)
    assert (rc, launches, batched, single) == (0, 1, 5, 0)


def test_valid_arguments_without_a_gpu_are_mpi_err_other(L):
    if L.msx_device_count() > 0:
        pytest.skip("GPU present")
    ins, ios = _layout([256, 256])
    a, b, c = _arrays(ins, ios, [64, 64])
    assert L.msx_reduce_local_batch_dev(a, b, c, 2, C.MPI_FLOAT, C.MPI_SUM, None) == C.MPI_ERR_OTHER
    assert L.msx_reduce_local_batch_dev(a, b, c, 2, C.MSX_BFLOAT16, C.MSX_SUM_WIDE, None) == C.MPI_ERR_OTHER
    # and the plan of the same arguments needs none
    assert _plan(L, ins, ios, [64, 64])[0] == 0


# ---- the plan's figures ------------------------------------------------------------

def _width(L):
    return _plan(L, [], [], [])[1]


def test_plan_of_small_aligned_segments(L):
    ins, ios = _layout([4 * KiB] * 100)
    rc, width, launches, batched, single = _plan(L, ins, ios, [1024] * 100)
    assert rc == 0 and width >= 16
    assert (batched, single) == (100, 0)
    assert launches == -(-100 // width)


def test_plan_cuts_fused_launches_at_width(L):
    w = _width(L)
    for n, want in ((1, 1), (w - 1, 1), (w, 1), (w + 1, 2), (2 * w, 2), (2 * w + 1, 3)):
        ins, ios = _layout([64] * n)
        assert _plan(L, ins, ios, [16] * n) == (0, w, want, n, 0), n


def test_plan_large_segments_are_launched_alone(L):
    sizes = [4 * KiB, LIMIT, 4 * KiB, LIMIT - 4, 4 * KiB]
    ins, ios = _layout(sizes)
    rc, w, launches, batched, single = _plan(L, ins, ios, [s // 4 for s in sizes])
    assert (rc, launches, batched, single) == (0, 2, 4, 1)        # 4 bytes short of 16 MiB is fused
    # the limit is in bytes per operand, whatever the element size
    for dt, esz in ((C.MPI_DOUBLE, 8), (C.MPI_INT8_T, 1), (C.MPI_C_DOUBLE_COMPLEX, 16), (C.MSX_FLOAT16, 2)):
        ins, ios = _layout([LIMIT, LIMIT])
        assert _plan(L, ins, ios, [LIMIT // esz, LIMIT // esz - 1], dt)[2:] == (2, 1, 1), esz


def test_plan_empty_segments_count_nowhere(L):
    w = _width(L)
    sizes = [0, 64, 0, 0, LIMIT, 0] + [64] * w + [0]
    ins, ios = _layout(sizes)
    rc, _, launches, batched, single = _plan(L, ins, ios, [s // 4 for s in sizes])
    assert (rc, launches, batched, single) == (0, 3, w + 1, 1)
    ins, ios = _layout([0, 0, 0])
    assert _plan(L, ins, ios, [0, 0, 0])[2:] == (0, 0, 0)


def test_plan_mutually_misaligned_segments(L):
    # in and inout at different offsets from 16-byte alignment: fused (as
    # scalars) when small, the realigning kernel of its own launch when large
    ins, ios = _layout([64, 64, 64])
    assert _plan(L, [ins[0] + 4, ins[1], ins[2]], [ios[0], ios[1] + 4, ios[2]], [16, 15, 16])[2:] == (1, 3, 0)
    ins, ios = _layout([1 * MiB + 64, 1 * MiB + 64, 64])
    assert _plan(L, [ins[0] + 4, ins[1] + 8, ins[2]], ios, [MiB // 4, MiB // 4, 16])[2:] == (3, 1, 2)
    # a common offset is no misalignment, at any size below the limit
    assert _plan(L, [ins[0] + 4, ins[1] + 8, ins[2]], [ios[0] + 4, ios[1] + 8, ios[2]],
                 [MiB // 4, MiB // 4, 16])[2:] == (1, 3, 0)
