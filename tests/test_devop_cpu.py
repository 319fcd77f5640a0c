"""Device-resident user ops (msx_op_create_device): handles, validation and
refusals, with ctypes callbacks as the device function.  No GPU needed."""
import ctypes

import numpy as np

import msx

C = msx.C

# MSX_Device_function: int (const void* in, void* inout, int64_t count,
#                           MPI_Datatype datatype, void* stream, void* state)
DF = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int,
                      ctypes.c_void_p, ctypes.c_void_p)
UF = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int),
                      ctypes.POINTER(ctypes.c_int))


def _device_op(L, fn, commute, state=None):
    op = ctypes.c_int(0)
    assert L.msx_op_create_device(fn, commute, state, ctypes.byref(op)) == 0, msx.last_error()
    return op


def test_null_function_is_an_argument_error(msxlib):
    L = msxlib
    op = ctypes.c_int(0)
    assert L.msx_op_create_device(None, 1, None, ctypes.byref(op)) == C.MPI_ERR_ARG
    fn = DF(lambda *a: 0)
    assert L.msx_op_create_device(fn, 1, None, None) == C.MPI_ERR_ARG


def test_handle_is_a_direct_user_op_and_reports_its_flag(msxlib):
    L = msxlib
    fn = DF(lambda *a: 0)
    c = ctypes.c_int(-1)
    for commute in (0, 1):
        op = _device_op(L, fn, commute)
        # type DIRECT (2) | kind MPID_OP (6), the pool of MPI_Op_create
        assert (op.value & 0xFC000000) == 0x98000000
        assert L.MPI_Op_commutative(op.value, ctypes.byref(c)) == 0 and c.value == commute
        assert L.MPI_Op_free(ctypes.byref(op)) == 0


def test_is_device_tells_the_kinds_apart(msxlib):
    L = msxlib
    fn = DF(lambda *a: 0)
    op = _device_op(L, fn, 1)
    assert L.msx_op_is_device(op.value) == 1
    hf = UF(lambda a, b, n, d: None)
    hop = ctypes.c_int(0)
    assert L.MPI_Op_create(hf, 1, ctypes.byref(hop)) == 0
    assert L.msx_op_is_device(hop.value) == 0
    assert L.msx_op_is_device(C.MPI_SUM) == 0
    assert L.msx_op_is_device(C.MPI_OP_NULL) == -1
    assert L.msx_op_is_device(0x98000000 | 0x3ffff) == -1
    assert L.MPI_Op_free(ctypes.byref(hop)) == 0
    assert L.MPI_Op_free(ctypes.byref(op)) == 0


def test_free_nulls_the_handle_and_a_freed_handle_is_invalid(msxlib):
    L = msxlib
    fn = DF(lambda *a: 0)
    op = _device_op(L, fn, 1)
    old = op.value
    assert L.MPI_Op_free(ctypes.byref(op)) == 0 and op.value == C.MPI_OP_NULL
    assert L.msx_op_is_device(old) == -1
    c = ctypes.c_int(-1)
    assert L.MPI_Op_commutative(old, ctypes.byref(c)) == C.MPI_ERR_OP
    a = np.arange(4, dtype=np.uint32)
    b = np.ones(4, dtype=np.uint32)
    assert L.MPI_Reduce_local(a.ctypes.data, b.ctypes.data, 4, C.MPI_UNSIGNED, old) == C.MPI_ERR_OP
    stale = ctypes.c_int(old)
    assert L.MPI_Op_free(ctypes.byref(stale)) == C.MPI_ERR_OP


def test_one_sided_calls_refuse_a_device_op(msxlib):
    L = msxlib
    fn = DF(lambda *a: 0)
    op = _device_op(L, fn, 1)
    buf = np.zeros(64, np.int32)
    src = np.arange(8, dtype=np.int32)
    win = ctypes.c_int()
    assert L.MPI_Win_create(buf.ctypes.data, 256, 4, C.MPI_INFO_NULL, C.MPI_COMM_WORLD, ctypes.byref(win)) == 0
    assert L.MPI_Win_set_errhandler(win, C.MPI_ERRORS_RETURN) == 0
    I = C.MPI_INT
    assert L.MPI_Accumulate(src.ctypes.data, 8, I, 0, 0, 8, I, op.value, win) == C.MPI_ERR_OP
    assert L.MPI_Win_free(ctypes.byref(win)) == 0
    assert L.MPI_Op_free(ctypes.byref(op)) == 0


def test_without_a_gpu_the_function_is_never_entered(msxlib):
    L = msxlib
    entered = []

    def f(*a):
        entered.append(a)
        return 0

    fn = DF(f)
    op = _device_op(L, fn, 0)
    a = np.arange(8, dtype=np.uint32)
    b = np.ones(8, dtype=np.uint32)
    if L.msx_device_count() == 0:
        assert L.MPI_Reduce_local(a.ctypes.data, b.ctypes.data, 8, C.MPI_UNSIGNED, op.value) == C.MPI_ERR_OTHER
        assert L.msx_reduce_local_dev(a.ctypes.data, b.ctypes.data, 8, C.MPI_UNSIGNED, op.value,
                                      None) == C.MPI_ERR_OTHER
        assert not entered and (b == 1).all()
    # argument checks come first, as for builtin ops, with or without a GPU
    assert L.MPI_Reduce_local(a.ctypes.data, a.ctypes.data, 8, C.MPI_UNSIGNED, op.value) == C.MPI_ERR_BUFFER
    assert L.msx_reduce_local_dev(a.ctypes.data, b.ctypes.data, -1, C.MPI_UNSIGNED, op.value, None) == C.MPI_ERR_COUNT
    assert L.msx_reduce_local_dev(None, b.ctypes.data, 8, C.MPI_UNSIGNED, op.value, None) == C.MPI_ERR_BUFFER
    assert not entered
    assert L.MPI_Op_free(ctypes.byref(op)) == 0
