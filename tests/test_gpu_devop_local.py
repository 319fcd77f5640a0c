"""GPU: device-resident user ops in one process -- the kernel kit
(include/msx_device_op.h) against numpy bit for bit, MPI_Reduce_local on device,
host and mixed operands, derived datatypes, msx_reduce_local_dev on a stream,
the state pointer and the error path.

The ops come from tests/devop/devop_ops.hip.  Every value is an integer
operation (wrapping 3 * in - inout) or an exact float selection (abs-max), so
every comparison is bit for bit."""
import ctypes
import os

import numpy as np
import pytest

import msx

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

C = msx.C
PAD = 64            # sentinel bytes on both sides of every operand (a multiple of 16)
SENT = 0x5A
OPS_LIB = os.path.join(msx.REPO_ROOT, "tests", "devop", "build", "libdevop_ops.so")


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    lib = msx.init(errors_return=True)
    assert lib.msx_device_count() > 0
    return lib


@pytest.fixture(scope="module")
def K(L):
    k = ctypes.CDLL(OPS_LIB)
    k.devop_kit_u32.restype = ctypes.c_int
    k.devop_kit_u32.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]
    k.devop_stats.restype = None
    k.devop_stats.argtypes = [ctypes.POINTER(ctypes.c_int64), ctypes.c_int]
    k.devop_set_stride2_n.restype = None
    k.devop_set_stride2_n.argtypes = [ctypes.c_int]
    return k


def _op(L, K, name, commute=0, state=None):
    op = ctypes.c_int(0)
    fn = ctypes.cast(getattr(K, name), ctypes.c_void_p)
    assert L.msx_op_create_device(fn, commute, state, ctypes.byref(op)) == 0, msx.last_error()
    return op


def _stats(K, reset=1):
    out = (ctypes.c_int64 * 3)()
    K.devop_stats(out, reset)
    return list(out)


class DevBuf:
    """`data` at byte offset `off` from 16-byte alignment, sentinels around it."""

    def __init__(self, data, off=0):
        self.raw = np.frombuffer(data.tobytes(), np.uint8)
        self.lo = PAD + off
        full = np.full(self.lo + self.raw.size + PAD, SENT, np.uint8)
        full[self.lo:self.lo + self.raw.size] = self.raw
        self.t = torch.from_numpy(full).pin_memory().cuda()      # page-locked source
        torch.cuda.synchronize()                                 # the library's streams do not order after torch's
        assert self.t.data_ptr() % 16 == 0
        self.ptr = self.t.data_ptr() + self.lo

    def read(self):
        h = torch.empty(self.t.numel(), dtype=torch.uint8).pin_memory()
        h.copy_(self.t)
        torch.cuda.synchronize()
        return h.numpy().copy()

    def check(self, exp, what):
        """the operand holds `exp` and nothing outside it changed"""
        full = self.read()
        want = np.full(full.size, SENT, np.uint8)
        e = np.frombuffer(exp.tobytes(), np.uint8)
        want[self.lo:self.lo + e.size] = e
        bad = np.nonzero(full != want)[0]
        assert bad.size == 0, f"{what}: {bad.size} bytes differ, first at {bad[0] - self.lo} (operand-relative)"


def nc(a, b, salt=0):
    """in (op) inout = 3 * in - inout + salt, wrapping in the arrays' type"""
    t = a.dtype.type
    return (a * t(3) - b + t(salt)).astype(a.dtype)


def _rand(rng, n, dtype):
    return rng.integers(0, np.iinfo(dtype).max, n, dtype=dtype, endpoint=True)


COUNTS = [0, 1, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025, 65537]
OFFSETS = [(0, 0), (4, 4), (12, 12), (0, 4), (8, 12)]


def test_kit_u32_matches_numpy_at_every_count_and_alignment(L, K):
    rng = np.random.default_rng(0xDE70)
    op = _op(L, K, "devop_nc_u32")
    for n in COUNTS:
        a, b = _rand(rng, n, np.uint32), _rand(rng, n, np.uint32)
        for oa, ob in OFFSETS:
            da, db = DevBuf(a, oa), DevBuf(b, ob)
            rc = L.msx_reduce_local_dev(da.ptr, db.ptr, n, C.MPI_UNSIGNED, op.value, None)
            assert rc == 0, msx.last_error()
            torch.cuda.synchronize()
            db.check(nc(a, b), f"count {n} offsets {oa},{ob} inout")
            da.check(a, f"count {n} offsets {oa},{ob} in")
    assert L.MPI_Op_free(ctypes.byref(op)) == 0


def _record_type(L, n, base):
    t = ctypes.c_int()
    assert L.MPI_Type_contiguous(n, base, ctypes.byref(t)) == 0
    assert L.MPI_Type_commit(ctypes.byref(t)) == 0
    return t


@pytest.mark.parametrize("size", [1, 2, 8, 16, 12])
def test_kit_every_element_size(L, K, size):
    rng = np.random.default_rng(size)
    name, dtype, per, mpi = {
        1: ("devop_nc_u8", np.uint8, 1, C.MPI_UNSIGNED_CHAR),
        2: ("devop_nc_u16", np.uint16, 1, C.MPI_UNSIGNED_SHORT),
        8: ("devop_nc_u64", np.uint64, 1, C.MPI_UNSIGNED_LONG_LONG),
        16: ("devop_nc_u64x2", np.uint64, 2, None),
        12: ("devop_nc_u32x3", np.uint32, 3, None),
    }[size]
    rec = None
    if mpi is None:
        rec = _record_type(L, per, C.MPI_UNSIGNED_LONG_LONG if size == 16 else C.MPI_UNSIGNED)
        mpi = rec.value
    op = _op(L, K, name)
    for n in (1, 17, 4099):
        a, b = _rand(rng, n * per, dtype), _rand(rng, n * per, dtype)
        # 12-byte records 4 bytes off alignment, the others aligned: both start on an element
        off = 4 if size == 12 else 0
        da, db = DevBuf(a, off), DevBuf(b, off)
        assert L.MPI_Reduce_local(da.ptr, db.ptr, n, mpi, op.value) == 0, msx.last_error()
        db.check(nc(a, b), f"size {size} count {n}")
    assert L.MPI_Op_free(ctypes.byref(op)) == 0
    if rec is not None:
        assert L.MPI_Type_free(ctypes.byref(rec)) == 0


# more than 1024 one-wave tiles: whole rounds of the XCD-run permutation, its
# unpermuted remainder, and a ragged tail
N_DRAM = (1024 + 37) * 256 + 3


@pytest.mark.parametrize("geometry", [2, 1])
def test_kit_forced_geometry(L, K, geometry):
    rng = np.random.default_rng(geometry)
    a, b = _rand(rng, N_DRAM, np.uint32), _rand(rng, N_DRAM, np.uint32)
    da, db = DevBuf(a), DevBuf(b)
    assert K.devop_kit_u32(da.ptr, db.ptr, N_DRAM, geometry, None) == 0
    torch.cuda.synchronize()
    db.check(nc(a, b), f"geometry {geometry}")
    da.check(a, f"geometry {geometry} in")


def test_kit_switches_geometry_above_16_mib(L, K):
    n = ((16 << 20) + (517 << 10) + 20) // 4
    rng = np.random.default_rng(16)
    a, b = _rand(rng, n, np.uint32), _rand(rng, n, np.uint32)
    da, db = DevBuf(a), DevBuf(b)
    assert K.devop_kit_u32(da.ptr, db.ptr, n, 0, None) == 0
    torch.cuda.synchronize()
    db.check(nc(a, b), "16 MiB + 517 KiB + 20 B")


def test_kit_rejects_bad_arguments(L, K):
    a = DevBuf(np.zeros(4, np.uint32))
    assert K.devop_kit_u32(a.ptr, a.ptr + 16, -1, 0, None) != 0
    assert K.devop_kit_u32(a.ptr, a.ptr + 16, 1, 3, None) != 0


def test_reduce_local_device_host_and_mixed_operands(L, K):
    """One call of the function with the full count each time, on device memory
    only -- host operands are staged to the GPU around it."""
    rng = np.random.default_rng(0x10CA1)
    op = _op(L, K, "devop_nc_u32")
    n = 70001
    a, b = _rand(rng, n, np.uint32), _rand(rng, n, np.uint32)
    exp = nc(a, b)
    # device, device
    da, db = DevBuf(a), DevBuf(b)
    _stats(K)
    assert L.MPI_Reduce_local(da.ptr, db.ptr, n, C.MPI_UNSIGNED, op.value) == 0, msx.last_error()
    assert _stats(K) == [1, n, 1]
    db.check(exp, "device operands")
    # pageable host, pageable host
    ha, hb = a.copy(), b.copy()
    assert L.MPI_Reduce_local(ha.ctypes.data, hb.ctypes.data, n, C.MPI_UNSIGNED, op.value) == 0, msx.last_error()
    assert _stats(K) == [1, n, 1]
    assert np.array_equal(hb, exp) and np.array_equal(ha, a)
    # device in, host inout
    hb = b.copy()
    assert L.MPI_Reduce_local(da.ptr, hb.ctypes.data, n, C.MPI_UNSIGNED, op.value) == 0, msx.last_error()
    assert _stats(K) == [1, n, 1]
    assert np.array_equal(hb, exp)
    # host in, device inout
    db = DevBuf(b)
    assert L.MPI_Reduce_local(ha.ctypes.data, db.ptr, n, C.MPI_UNSIGNED, op.value) == 0, msx.last_error()
    assert _stats(K) == [1, n, 1]
    db.check(exp, "host in, device inout")
    assert L.MPI_Op_free(ctypes.byref(op)) == 0


def _stride2_type(L, K, n):
    t = ctypes.c_int()
    assert L.MPI_Type_vector(n, 1, 2, C.MPI_UNSIGNED, ctypes.byref(t)) == 0
    assert L.MPI_Type_commit(ctypes.byref(t)) == 0
    K.devop_set_stride2_n(n)
    return t


def test_reduce_local_derived_type_keeps_the_gaps(L, K):
    rng = np.random.default_rng(0x571D)
    n = 3001
    t = _stride2_type(L, K, n)
    op = _op(L, K, "devop_stride2_u32")
    a, b = _rand(rng, 2 * n - 1, np.uint32), _rand(rng, 2 * n - 1, np.uint32)
    exp = b.copy()
    exp[0::2] = nc(a[0::2], b[0::2])
    da, db = DevBuf(a), DevBuf(b)
    _stats(K)
    assert L.MPI_Reduce_local(da.ptr, db.ptr, 1, t.value, op.value) == 0, msx.last_error()
    assert _stats(K) == [1, 1, 1]
    db.check(exp, "stride2 on device")
    ha, hb = a.copy(), b.copy()
    assert L.MPI_Reduce_local(ha.ctypes.data, hb.ctypes.data, 1, t.value, op.value) == 0, msx.last_error()
    assert _stats(K) == [1, 1, 1]
    assert np.array_equal(hb, exp)
    assert L.MPI_Op_free(ctypes.byref(op)) == 0
    assert L.MPI_Type_free(ctypes.byref(t)) == 0


def test_reduce_local_dev_is_stream_ordered(L, K):
    """Enqueued on the caller's stream: a dependent torch op on that stream sees
    the result with no synchronisation in between."""
    rng = np.random.default_rng(0x57E4)
    n = 1 << 20
    a, b = _rand(rng, n, np.uint32), _rand(rng, n, np.uint32)
    op = _op(L, K, "devop_nc_u32")
    pa = torch.from_numpy(a.view(np.int32)).pin_memory()
    pb = torch.from_numpy(b.view(np.int32)).pin_memory()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        ta = pa.to("cuda", non_blocking=True)
        tb = pb.to("cuda", non_blocking=True)
        rc = L.msx_reduce_local_dev(ta.data_ptr(), tb.data_ptr(), n, C.MPI_UNSIGNED, op.value,
                                    ctypes.c_void_p(s.cuda_stream))
        out = tb + 1                        # depends on the combine, same stream, no sync before it
        res = torch.empty(n, dtype=torch.int32).pin_memory()
        res.copy_(out, non_blocking=True)
    assert rc == 0, msx.last_error()
    s.synchronize()
    assert np.array_equal(res.numpy().view(np.uint32), nc(a, b) + np.uint32(1))
    assert L.MPI_Op_free(ctypes.byref(op)) == 0


def test_state_reaches_the_function(L, K):
    rng = np.random.default_rng(0x5A17)
    salt = ctypes.c_uint32(0x9E3779B9)
    op = _op(L, K, "devop_nc_u32", 0, ctypes.cast(ctypes.pointer(salt), ctypes.c_void_p))
    n = 1027
    a, b = _rand(rng, n, np.uint32), _rand(rng, n, np.uint32)
    da, db = DevBuf(a, 4), DevBuf(b, 4)
    assert L.MPI_Reduce_local(da.ptr, db.ptr, n, C.MPI_UNSIGNED, op.value) == 0, msx.last_error()
    db.check(nc(a, b, salt.value), "salted")
    assert L.MPI_Op_free(ctypes.byref(op)) == 0


def test_a_failing_function_fails_the_call(L, K):
    op = _op(L, K, "devop_fail")
    a, b = np.arange(100, dtype=np.uint32), np.full(100, 7, np.uint32)
    da, db = DevBuf(a), DevBuf(b)
    assert L.MPI_Reduce_local(da.ptr, db.ptr, 100, C.MPI_UNSIGNED, op.value) == C.MPI_ERR_ARG
    db.check(b, "inout after a failed call")
    hb = b.copy()
    assert L.MPI_Reduce_local(a.ctypes.data, hb.ctypes.data, 100, C.MPI_UNSIGNED, op.value) == C.MPI_ERR_ARG
    assert np.array_equal(hb, b)
    assert L.MPI_Op_free(ctypes.byref(op)) == 0


def test_absmax_is_exact(L, K):
    rng = np.random.default_rng(0xAB5)
    n = 100003
    a = rng.uniform(-1e6, 1e6, n).astype(np.float32)
    b = rng.uniform(-1e6, 1e6, n).astype(np.float32)
    a[:4] = [0.0, -0.0, np.float32(-3.5), np.float32(1e-40)]
    b[:4] = [-0.0, 0.0, np.float32(3.5), np.float32(-1e-41)]
    op = _op(L, K, "devop_absmax_f32", 1)
    da, db = DevBuf(a), DevBuf(b)
    assert L.MPI_Reduce_local(da.ptr, db.ptr, n, C.MPI_FLOAT, op.value) == 0, msx.last_error()
    db.check(np.maximum(np.abs(a), np.abs(b)), "abs-max")
    assert L.MPI_Op_free(ctypes.byref(op)) == 0
