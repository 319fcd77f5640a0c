"""CPU: the 16-bit float datatypes MSX_FLOAT16 / MSX_BFLOAT16 (extensions of
include/msx.h) in the tables, the datatype engine and the headers, plus a
self-test of the numpy reference the GPU tests hold the kernels to
(tests/_half_ref.py).  No compute call here needs a GPU."""
import ctypes
import json
import os
import subprocess

import numpy as np

import msx
import _half_ref as R

C = msx.C
c_int, c_i64 = ctypes.c_int, ctypes.c_int64
u32 = lambda v: v & 0xFFFFFFFF
HALF = (("MSX_FLOAT16", 0x4C000250), ("MSX_BFLOAT16", 0x4C000251))
LEGAL = ("MPI_MAX", "MPI_MIN", "MPI_SUM", "MPI_PROD")
ILLEGAL = ("MPI_LAND", "MPI_BAND", "MPI_LOR", "MPI_BOR", "MPI_LXOR", "MPI_BXOR", "MPI_MINLOC", "MPI_MAXLOC",
           "MPI_REPLACE", "MPI_NO_OP")


def test_handles_values_and_no_collision_with_mpi_h():
    L = msx.lib()
    for name, val in HALF:
        assert u32(getattr(C, name)) == val
        assert (val >> 8) & 0xFF == 2 and val >> 16 == 0x4C00          # builtin layout, size byte 02
        assert L.msx_type_size(getattr(C, name)) == 2
    with open(os.path.join(msx.REPO_ROOT, "tests", "golden", "mpi_h_constants.json")) as f:
        golden = json.load(f)["constants"]
    taken = {u32(v) for v in golden.values()}
    taken |= {u32(v) for k, v in vars(C).items() if k.startswith("MPI_") and isinstance(v, int)}
    for name, val in HALF:
        assert val not in taken, name
    assert C.MPI_REAL2 == C.MPI_DATATYPE_NULL                           # mpi.h unchanged
    with open(os.path.join(msx.INCLUDE_DIR, "mpi.h")) as f:
        txt = f.read()
    assert "MSX_FLOAT16" not in txt and "MSX_BFLOAT16" not in txt


def test_op_legality_is_max_min_sum_prod_only():
    L = msx.lib()
    for name, _ in HALF:
        dt = getattr(C, name)
        for op in LEGAL:
            assert L.msx_op_check(getattr(C, op), dt) == C.MPI_SUCCESS, (op, name)
        for op in ILLEGAL:
            assert L.msx_op_check(getattr(C, op), dt) == C.MPI_ERR_OP, (op, name)
    # floats of the reference keep their (non-strict) logical ops
    assert L.msx_op_check(C.MPI_LAND, C.MPI_FLOAT) == C.MPI_SUCCESS


def test_op_table_entry_rejects_illegal_pair_without_touching_inout(msxlib):
    L = msxlib
    UF = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(c_int), ctypes.POINTER(c_int))
    L.msx_op_table.restype = ctypes.c_void_p
    L.msx_op_table.argtypes = [c_int]
    L.msx_op_errno.restype = c_int
    a = np.arange(8, dtype=np.uint16)
    b = np.full(8, 5, dtype=np.uint16)
    for name, _ in HALF:
        L.msx_op_errno_reset()
        UF(L.msx_op_table(C.MPI_LAND))(a.ctypes.data, b.ctypes.data, ctypes.byref(c_int(8)),
                                        ctypes.byref(c_int(getattr(C, name))))
        assert L.msx_op_errno() == C.MPI_ERR_OP and (b == 5).all()
    L.msx_op_errno_reset()


def test_type_size_extent_envelope(msxlib):
    L = msxlib
    for name, _ in HALF:
        dt = getattr(C, name)
        sz = c_int(-1)
        assert L.MPI_Type_size(dt, ctypes.byref(sz)) == 0 and sz.value == 2
        lb, ext = c_i64(-1), c_i64(-1)
        assert L.MPI_Type_get_extent(dt, ctypes.byref(lb), ctypes.byref(ext)) == 0
        assert (lb.value, ext.value) == (0, 2)
        assert L.MPI_Type_get_true_extent(dt, ctypes.byref(lb), ctypes.byref(ext)) == 0
        assert (lb.value, ext.value) == (0, 2)
        ni, na, nt, comb = c_int(-1), c_int(-1), c_int(-1), c_int(-1)
        assert L.MPI_Type_get_envelope(dt, ctypes.byref(ni), ctypes.byref(na), ctypes.byref(nt),
                                       ctypes.byref(comb)) == 0
        assert (ni.value, na.value, nt.value, comb.value) == (0, 0, 0, C.MPI_COMBINER_NAMED)


def test_derived_types_over_half_and_pack_size(msxlib):
    L = msxlib
    for name, _ in HALF:
        dt = getattr(C, name)
        v = c_int()
        assert L.MPI_Type_vector(5, 3, 7, dt, ctypes.byref(v)) == 0, msx.last_error()
        assert L.MPI_Type_commit(ctypes.byref(v)) == 0
        sz, lb, ext = c_int(), c_i64(), c_i64()
        assert L.MPI_Type_size(v.value, ctypes.byref(sz)) == 0 and sz.value == 5 * 3 * 2
        assert L.MPI_Type_get_extent(v.value, ctypes.byref(lb), ctypes.byref(ext)) == 0
        assert (lb.value, ext.value) == (0, (4 * 7 + 3) * 2)
        ps = c_int()
        assert L.MPI_Pack_size(4, v.value, C.MPI_COMM_WORLD, ctypes.byref(ps)) == 0 and ps.value == 4 * 30
        ni, na, nt, comb = c_int(), c_int(), c_int(), c_int()
        assert L.MPI_Type_get_envelope(v.value, ctypes.byref(ni), ctypes.byref(na), ctypes.byref(nt),
                                       ctypes.byref(comb)) == 0
        assert comb.value == C.MPI_COMBINER_VECTOR and nt.value == 1
        ints, aints, types = (c_int * 3)(), (c_i64 * 1)(), (c_int * 1)()
        assert L.MPI_Type_get_contents(v.value, 3, 0, 1, ints, aints, types) == 0
        assert list(ints) == [5, 3, 7] and types[0] == dt
        sizes, subs, starts = (c_int * 2)(6, 10), (c_int * 2)(3, 4), (c_int * 2)(1, 5)
        s = c_int()
        assert L.MPI_Type_create_subarray(2, sizes, subs, starts, C.MPI_ORDER_C, dt, ctypes.byref(s)) == 0
        assert L.MPI_Type_commit(ctypes.byref(s)) == 0
        assert L.MPI_Type_size(s.value, ctypes.byref(sz)) == 0 and sz.value == 3 * 4 * 2
        assert L.MPI_Type_get_extent(s.value, ctypes.byref(lb), ctypes.byref(ext)) == 0
        assert (lb.value, ext.value) == (0, 6 * 10 * 2)
        assert L.MPI_Pack_size(2, s.value, C.MPI_COMM_WORLD, ctypes.byref(ps)) == 0 and ps.value == 48
        assert L.MPI_Pack_size(3, dt, C.MPI_COMM_WORLD, ctypes.byref(ps)) == 0 and ps.value == 6
        for t in (s, v):
            assert L.MPI_Type_free(ctypes.byref(t)) == 0


def test_user_op_sees_plain_two_byte_elements(msxlib):
    L = msxlib
    UF = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(c_int), ctypes.POINTER(c_int))
    seen = []

    def bxor(invec, inoutvec, n, dt):
        seen.append((n[0], dt[0]))
        x = np.ctypeslib.as_array((ctypes.c_uint16 * n[0]).from_address(invec))
        y = np.ctypeslib.as_array((ctypes.c_uint16 * n[0]).from_address(inoutvec))
        y[:] = x ^ y

    fn = UF(bxor)
    op = c_int()
    assert L.MPI_Op_create(fn, 1, ctypes.byref(op)) == 0
    a = np.arange(9, dtype=np.uint16) * 257
    b = np.full(9, 0x3C00, np.uint16)
    assert L.MPI_Reduce_local(a.ctypes.data, b.ctypes.data, 9, C.MSX_BFLOAT16, op.value) == 0, msx.last_error()
    assert (b == (a ^ 0x3C00)).all() and seen == [(9, C.MSX_BFLOAT16)]
    assert L.MPI_Op_free(ctypes.byref(op)) == 0


def test_builtin_reduce_without_gpu_fails_loudly(msxlib):
    a = np.full(8, 0x3C00, np.uint16)
    b = np.full(8, 0x4000, np.uint16)
    # an illegal pair is refused before any device is needed
    assert msxlib.MPI_Reduce_local(a.ctypes.data, b.ctypes.data, 8, C.MSX_FLOAT16, C.MPI_BAND) == C.MPI_ERR_OP
    if msxlib.msx_device_count() == 0:
        rc = msxlib.MPI_Reduce_local(a.ctypes.data, b.ctypes.data, 8, C.MSX_FLOAT16, C.MPI_SUM)
        assert rc == C.MPI_ERR_OTHER and "no usable MI355X" in msx.last_error()
        assert (b == 0x4000).all()


def test_plain_c_file_naming_both_constants_compiles(tmp_path):
    src = tmp_path / "half.c"
    src.write_text("""
        #include "msx.h"
        static const MPI_Datatype kinds[2] = {MSX_FLOAT16, MSX_BFLOAT16};
        int half_sizes(void)
        {
            switch (kinds[0]) { case MSX_FLOAT16: break; case MSX_BFLOAT16: return -1; default: return -2; }
            return msx_type_size(kinds[0]) + msx_type_size(kinds[1]);
        }
    """)
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", msx.INCLUDE_DIR, "-c",
                    str(src), "-o", str(tmp_path / "half.o")], check=True)


# ---- the numpy reference on known answers ----------------------------------------
def _u16(*v):
    return np.array(v, np.uint16)


def test_reference_rounds_to_nearest_even_both_ways():
    # bf16: 1 + 2^-8 is halfway between 1 (even) and 1 + 2^-7 (odd): down;
    # (1 + 2^-7) + 2^-8 is halfway between odd 0x3F81 and even 0x3F82: up
    assert R.combine("MPI_SUM", "MSX_BFLOAT16", _u16(0x3F80, 0x3F81), _u16(0x3B80, 0x3B80)).tolist() == [0x3F80, 0x3F82]
    # fp16: 1 + 2^-11 -> 1 (even), (1 + 2^-10) + 2^-11 -> 1 + 2^-9 (even)
    assert R.combine("MPI_SUM", "MSX_FLOAT16", _u16(0x3C00, 0x3C01), _u16(0x1000, 0x1000)).tolist() == [0x3C00, 0x3C02]
    # just above the tie rounds up: bf16 1 + (2^-8 + 2^-15)
    assert R.n_bf16(np.array([0x3F808001], np.uint32).view(np.float32)).tolist() == [0x3F81]
    assert R.n_bf16(np.array([0x3F808000, 0x3F818000], np.uint32).view(np.float32)).tolist() == [0x3F80, 0x3F82]


def test_reference_overflow_subnormals_and_default_nan():
    for dt, mx, inf in (("MSX_FLOAT16", 0x7BFF, 0x7C00), ("MSX_BFLOAT16", 0x7F7F, 0x7F80)):
        assert R.combine("MPI_SUM", dt, _u16(mx, 0x8000 | mx), _u16(mx, 0x8000 | mx)).tolist() == [inf, 0x8000 | inf]
        assert R.combine("MPI_PROD", dt, _u16(mx), _u16(mx)).tolist() == [inf]
        # the smallest subnormal survives 1 * x and x + 0, and x + x is exact
        assert R.combine("MPI_PROD", dt, _u16(0x0001), _u16(0x3C00 if dt == "MSX_FLOAT16" else 0x3F80)).tolist() == [1]
        assert R.combine("MPI_SUM", dt, _u16(0x0001, 0x0001), _u16(0x0000, 0x0001)).tolist() == [1, 2]
        # inf - inf and 0 * inf: the sign-set default NaN
        assert R.combine("MPI_SUM", dt, _u16(inf), _u16(0x8000 | inf)).tolist() == [R.DNAN[dt]]
        assert R.combine("MPI_PROD", dt, _u16(0x0000), _u16(inf)).tolist() == [R.DNAN[dt]]
    # fp16: half of the smallest subnormal ties to even zero, three halves to 2
    assert R.combine("MPI_PROD", "MSX_FLOAT16", _u16(0x0001, 0x0003), _u16(0x3800, 0x3800)).tolist() == [0, 2]
    # a bf16 product in fp32's subnormal range is rounded from the fp32 result
    a = _u16(0x0080)                                                     # 2^-126
    assert R.combine("MPI_PROD", "MSX_BFLOAT16", a, _u16(0x3F00)).tolist() == [0x0040]    # 2^-127


def test_reference_nan_rule_signalling_nan_in_each_role():
    for dt, inf in (("MSX_FLOAT16", 0x7C00), ("MSX_BFLOAT16", 0x7F80)):
        q = R.QBIT[dt]
        snan_a, snan_b, qnan = inf | 1, 0x8000 | inf | 2, inf | q | 3
        one = 0x3C00 if dt == "MSX_FLOAT16" else 0x3F80
        for op in ("MPI_SUM", "MPI_PROD"):
            # inout a NaN: inout's bits, quieted -- whatever `in` is
            assert R.combine(op, dt, _u16(snan_a, snan_a, qnan), _u16(one, snan_b, snan_b)).tolist() == \
                [snan_a | q, snan_a | q, qnan]
            # only `in` a NaN: in's bits, quieted
            assert R.combine(op, dt, _u16(one), _u16(snan_b)).tolist() == [snan_b | q]
        # MAX / MIN: any NaN operand yields `in`, bits unchanged; (+0, -0) yields `in`
        for op in ("MPI_MAX", "MPI_MIN"):
            assert R.combine(op, dt, _u16(snan_a, one, 0x0000, 0x8000), _u16(one, snan_b, 0x8000, 0x0000)).tolist() == \
                [one, snan_b, 0x8000, 0x0000]
        assert R.combine("MPI_MAX", dt, _u16(one), _u16(0x8000 | one)).tolist() == [one]
        assert R.combine("MPI_MIN", dt, _u16(one), _u16(0x8000 | one)).tolist() == [0x8000 | one]


def test_reference_partners_and_tree_walk():
    for dt in R.TYPES:
        p = R.partners(dt)
        assert p.size == 64 and p.dtype == np.uint16
        inf = 0x7C00 if dt == "MSX_FLOAT16" else 0x7F80
        for must in (0, 0x8000, inf, 0x8000 | inf, 1, inf - 1, inf | 1):
            assert must in p.tolist()
    # the tree rounds at every node: (a + b) + c with bf16 1, 2^-8, 2^-8 stays 1
    # (each partial ties to even), while the fp32 sum 1 + 2^-7 would be 0x3F81
    s = [_u16(0x3F80), _u16(0x3B80), _u16(0x3B80)]
    assert R.tree("MPI_SUM", "MSX_BFLOAT16", s, 3, 0, 0, 1).tolist() == [0x3F80]
    four = [_u16(0x3F80), None, _u16(0x3B80), None, _u16(0x3B80), None, _u16(0x3B80), None]
    # ((1 + e) + (e + e)): 1 + e -> 1, e + e = 2e, 1 + 2e = 0x3F81
    assert R.tree("MPI_SUM", "MSX_BFLOAT16", four, 4, 0, 4, 0).tolist() == [0x3F81]
