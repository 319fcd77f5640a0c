"""CPU, no GPU: msx_accumulate_widen_dev / msx_accumulate_widen_plan
(include/msx.h): the two symbols, the order of the host-side checks, the plan's
figures, and the reference the GPU test holds the kernels to
(tests/_widen_ref.py).

Every check-order case breaks one check and at least one later one; the class
that comes back names the check that ran first.  The plan is a pure function
of its arguments, so it runs without a GPU; the real call is driven only into
its checks (null or fake addresses are never dereferenced there) and, without
a GPU, to MPI_ERR_OTHER."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import msx
import _widen_ref as WR
from test_dtype_cpu import build_lib, free_all

C = msx.C
vp, i64, c_int = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int

BASE = 0x7F0000000000          # a fake, 16-byte aligned device address
FAR = BASE + (1 << 36)
BF, HF, F = C.MSX_BFLOAT16, C.MSX_FLOAT16, C.MPI_FLOAT


@pytest.fixture(scope="module")
def L():
    return msx.init(errors_return=True)


@pytest.fixture(scope="module")
def T(L):
    """Committed types by name, freed at the end; `raw` stays uncommitted."""
    keep = []
    bf, hf, f, b = ("basic", BF), ("basic", HF), ("basic", F), ("basic", C.MPI_BYTE)
    recipes = {
        "bv": ("vector", 5, 3, 7, bf),                    # 15 bf16 in 5 blocks of 3
        "hv": ("vector", 5, 3, 7, hf),
        "bc10": ("contig", 10, bf),
        "bix": ("indexed", [3, 1, 4, 1, 5], [0, 5, 7, 13, 16], bf),          # 14 elements, irregular
        "fsub": ("subarray", [6, 9], [3, 5], [2, 1], True, f),               # 15 fp32
        "fv3": ("vector", 37, 1, 3, f),
        "fc10": ("contig", 10, f),
        "dv": ("vector", 5, 3, 7, ("basic", C.MPI_DOUBLE)),
        "pair": ("vector", 4, 1, 2, ("basic", C.MPI_FLOAT_INT)),
        "mixed_o": ("struct", [1, 1], [0, 2], [("basic", C.MPI_INT8_T), bf]),
        "mixed_t": ("struct", [1, 1], [0, 8], [("basic", C.MPI_INT8_T), f]),
        # Structs whose data bytes cut through where an element would be: two single bytes with a gap
        # on the origin side, two 2-byte halves on the target side.  The public constructors only
        # build type maps out of whole basic elements, so a struct reaches the split-element rule's
        # class (MPI_ERR_TYPE) through its element type, MPI_BYTE, which is not the kind asked for.
        "bytes2": ("struct", [1, 1], [0, 2], [b, b]),
        "bytes4": ("struct", [2, 2], [0, 4], [b, b]),
    }
    out = {}
    for name, r in recipes.items():
        h = build_lib(L, r, keep)
        x = c_int(h)
        assert L.MPI_Type_commit(ctypes.byref(x)) == 0
        out[name] = h
    out["raw"] = build_lib(L, ("vector", 3, 1, 2, bf), keep)
    yield out
    free_all(L, keep)


@pytest.fixture(scope="module")
def user_op(L):
    UF = ctypes.CFUNCTYPE(None, vp, vp, ctypes.POINTER(c_int), ctypes.POINTER(c_int))
    fn = UF(lambda a, b, n, d: None)
    op = c_int()
    assert L.MPI_Op_create(fn, 1, ctypes.byref(op)) == 0
    yield op.value
    assert L.MPI_Op_free(ctypes.byref(op)) == 0
    del fn


@pytest.fixture(scope="module")
def device_op(L):
    DF = ctypes.CFUNCTYPE(c_int, vp, vp, i64, c_int, vp, vp)
    fn = DF(lambda *_: 0)
    op = c_int()
    assert L.msx_op_create_device(fn, 1, None, ctypes.byref(op)) == 0
    yield op.value
    assert L.MPI_Op_free(ctypes.byref(op)) == 0
    del fn


def _plan(L, oc, odt, tc, tdt, op):
    """(rc, elements, path)"""
    n, path = i64(-7), c_int(-7)
    rc = L.msx_accumulate_widen_plan(oc, odt, tc, tdt, op, ctypes.byref(n), ctypes.byref(path))
    return rc, n.value, path.value


def _both(L, oc, odt, tc, tdt, op, origin=None, target=None):
    """The class both entry points return for arguments that fail a check."""
    rc = L.msx_accumulate_widen_dev(origin, oc, odt, target, tc, tdt, op, None)
    err = msx.last_error()
    assert rc != 0
    assert _plan(L, oc, odt, tc, tdt, op)[0] == rc
    return rc, err


# ---- the symbols and the reference ---------------------------------------------------

def test_both_symbols_are_exported_and_declared(L):
    with open(os.path.join(msx.INCLUDE_DIR, "msx.h")) as f:
        txt = f.read()
    for name in ("msx_accumulate_widen_dev", "msx_accumulate_widen_plan"):
        assert hasattr(L, name)
        assert getattr(L, name).argtypes is not None
        assert name in msx.exported_symbols()
        assert re.search(r"^int %s\(" % name, txt, re.M)


def test_a_pedantic_c99_file_naming_both_functions_compiles(tmp_path):
    src = tmp_path / "widen.c"
    src.write_text(
        '#include "mpi.h"\n#include "msx.h"\n'
        "int (*const a)(const void*, int64_t, MPI_Datatype, void*, int64_t, MPI_Datatype, MPI_Op, void*) =\n"
        "    msx_accumulate_widen_dev;\n"
        "int (*const b)(int64_t, MPI_Datatype, int64_t, MPI_Datatype, MPI_Op, int64_t*, int*) =\n"
        "    msx_accumulate_widen_plan;\n"
        "int use(void* o, void* t)\n{\n    int64_t n; int path;\n"
        "    return msx_accumulate_widen_plan(4, MSX_BFLOAT16, 4, MPI_FLOAT, MPI_SUM, &n, &path)\n"
        "         + msx_accumulate_widen_dev(o, 4, MSX_FLOAT16, t, 4, MPI_FLOAT, MPI_MAX, 0);\n}\n")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", msx.INCLUDE_DIR, "-c",
                        str(src), "-o", str(tmp_path / "widen.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_reference_widening_is_exact_and_injective():
    WR.self_test()


def test_the_reference_combine_is_the_oracles_fp32_op():
    o = np.array([0x3F80, 0x4000, 0x7FC1, 0x7F81, 0xFF80], np.uint16)            # bf16: 1, 2, qNaN, sNaN, -inf
    t = np.array([0x40400000, 0x7FA00001, 0x3F800000, 0x3F800000, 0x7F800000], np.uint32)
    got = WR.combine("MPI_SUM", "MSX_BFLOAT16", o, t)
    # 3 + 1; the target's sNaN quieted; the origin's qNaN; its sNaN quieted; inf - inf: the default NaN
    assert [hex(v) for v in got] == ["0x40800000", "0x7fe00001", "0x7fc10000", "0x7fc10000", "0xffc00000"]
    got = WR.combine("MPI_MAX", "MSX_BFLOAT16", o, t)
    # 3 > 1; NaN > x is false: `in`, here W(origin), unquieted
    assert [hex(v) for v in got] == ["0x40400000", "0x40000000", "0x7fc10000", "0x7f810000", "0x7f800000"]
    assert np.array_equal(WR.combine("MPI_REPLACE", "MSX_BFLOAT16", o, t), o.astype(np.uint32) << 16)


# ---- the order of the checks -------------------------------------------------------

def test_counts_come_first(L, T):
    # check 1, with a bad datatype, a bad op, truncation and null buffers behind it
    for oc, tc in ((-1, 1), (1, -1), (-5, -5)):
        assert _both(L, oc, 0x1234, tc, T["raw"], 0x1234)[0] == C.MPI_ERR_COUNT
        assert _both(L, oc, T["bv"], tc, T["fsub"], C.MPI_BAND)[0] == C.MPI_ERR_COUNT


def test_datatypes_come_before_the_op(L, T, user_op):
    # check 2, with a bad op, truncation, wrong element types and null buffers behind it
    for op in (0x1234, user_op, C.MSX_SUM_WIDE, C.MPI_BAND, C.MPI_SUM):
        assert _both(L, 9, 0x1234, 1, T["dv"], op)[0] == C.MPI_ERR_TYPE
        assert _both(L, 9, T["bv"], 1, C.MPI_DATATYPE_NULL, op)[0] == C.MPI_ERR_TYPE
        rc, err = _both(L, 9, T["raw"], 1, T["dv"], op)
        assert rc == C.MPI_ERR_TYPE and "not committed" in err


def test_the_op_comes_before_truncation_and_the_element_types(L, T, user_op, device_op):
    # check 3: 9 x 15 bf16 into 1 x 15 doubles behind it (truncation, a wrong target, null buffers)
    a = (9, T["bv"], 1, T["dv"])
    assert _both(L, *a, 0x1234)[0] == C.MPI_ERR_OP
    assert _both(L, *a, C.MPI_OP_NULL)[0] == C.MPI_ERR_OP
    for op in (user_op, device_op):
        rc, err = _both(L, *a, op)
        assert rc == C.MPI_ERR_OP and "builtin ops only" in err
    rc, err = _both(L, *a, C.MSX_SUM_WIDE)
    assert rc == C.MPI_ERR_OP and "MSX_SUM_WIDE" in err
    # also on a pair every other check accepts
    good = (4, BF, 4, F)
    assert _plan(L, *good, C.MPI_SUM) == (0, 4, 1)
    assert _both(L, *good, C.MSX_SUM_WIDE)[0] == C.MPI_ERR_OP
    assert _both(L, *good, user_op)[0] == C.MPI_ERR_OP
    for name in ("MPI_BAND", "MPI_BOR", "MPI_BXOR", "MPI_LAND", "MPI_LOR", "MPI_LXOR", "MPI_MAXLOC", "MPI_MINLOC"):
        rc, err = _both(L, *good, getattr(C, name))
        assert rc == C.MPI_ERR_OP and name in err, (name, err)
        assert _both(L, *a, getattr(C, name))[0] == C.MPI_ERR_OP


def test_truncation_comes_before_the_element_types(L, T):
    # check 4: twice the origin's bytes count; wrong element types and null buffers behind it.
    # 2 x 30 origin bytes widen to the 120 of 15 doubles: no truncation, so check 6 answers
    assert _both(L, 2, T["bv"], 1, T["dv"], C.MPI_SUM)[0] == C.MPI_ERR_TYPE
    assert _plan(L, 2, T["bv"], 1, T["dv"], C.MPI_NO_OP) == (0, 30, 0)
    for op in (C.MPI_SUM, C.MPI_REPLACE, C.MPI_NO_OP):
        rc, err = _both(L, 3, T["bv"], 1, T["dv"], op)                 # 2 x 90 origin bytes into 120
        assert rc == C.MPI_ERR_TRUNCATE and "90" in err and "120" in err
    assert _both(L, 5, BF, 4, F, C.MPI_SUM)[0] == C.MPI_ERR_TRUNCATE   # 20 widened bytes into 16
    assert _both(L, 1, BF, 0, F, C.MPI_SUM)[0] == C.MPI_ERR_TRUNCATE
    assert _both(L, 4, F, 4, F, C.MPI_SUM)[0] == C.MPI_ERR_TRUNCATE    # equal data bytes do not do
    assert _both(L, 1, T["bv"], 14, F, C.MPI_SUM)[0] == C.MPI_ERR_TRUNCATE
    assert _plan(L, 1, T["bv"], 15, F, C.MPI_SUM)[0] == 0
    # data bytes beyond 2^62
    assert _both(L, 1 << 62, BF, 1 << 62, F, C.MPI_SUM)[0] == C.MPI_ERR_COUNT
    assert _plan(L, 1 << 60, BF, 1 << 60, F, C.MPI_SUM) == (0, 1 << 60, 1)


def test_nothing_to_do_succeeds_before_the_element_types_and_the_buffers(L, T):
    # check 5: wrong element types, a type without an element type and null buffers behind it
    for odt, tdt, op in ((T["bv"], T["dv"], C.MPI_SUM), (F, F, C.MPI_MAX), (T["pair"], T["mixed_t"], C.MPI_REPLACE)):
        assert L.msx_accumulate_widen_dev(None, 0, odt, None, 3, tdt, op, None) == 0
        assert L.msx_accumulate_widen_dev(None, 0, odt, None, 0, tdt, op, None) == 0
        assert _plan(L, 0, odt, 3, tdt, op) == (0, 0, 0)
    assert L.msx_accumulate_widen_dev(None, 1, T["mixed_o"], None, 2, T["fv3"], C.MPI_NO_OP, None) == 0
    assert L.msx_accumulate_widen_dev(None, 1, T["bv"], None, 1, T["dv"], C.MPI_NO_OP, None) == 0
    assert _plan(L, 1, T["bv"], 1, T["dv"], C.MPI_NO_OP) == (0, 15, 0)
    assert _plan(L, 4, BF, 4, F, C.MPI_NO_OP) == (0, 4, 0)


def test_element_types_come_before_the_buffers(L, T):
    # check 6 with null buffers behind it, for an op and for MPI_REPLACE alike
    for op in (C.MPI_SUM, C.MPI_MIN, C.MPI_REPLACE):
        rc, err = _both(L, 4, F, 8, F, op)
        assert rc == C.MPI_ERR_TYPE and "neither MSX_FLOAT16 nor MSX_BFLOAT16" in err
        rc, err = _both(L, 4, BF, 8, BF, op)
        assert rc == C.MPI_ERR_TYPE and "not 4-byte floats" in err
        assert _both(L, 4, HF, 8, HF, op)[0] == C.MPI_ERR_TYPE
        rc, err = _both(L, 4, BF, 4, C.MPI_DOUBLE, op)
        assert rc == C.MPI_ERR_TYPE and "not 4-byte floats" in err
        assert _both(L, 1, T["bv"], 1, T["dv"], op)[0] == C.MPI_ERR_TYPE
        assert _both(L, 4, BF, 4, C.MPI_INT, op)[0] == C.MPI_ERR_TYPE
        assert _both(L, 4, C.MPI_SHORT, 4, F, op)[0] == C.MPI_ERR_TYPE
        # no single element type: the pair types, mixed structs
        rc, err = _both(L, 1, BF, 1, T["pair"], op)
        assert rc == C.MPI_ERR_TYPE and "no single basic element type" in err
        assert _both(L, 1, BF, 1, C.MPI_FLOAT_INT, op)[0] == C.MPI_ERR_TYPE
        rc, err = _both(L, 1, T["mixed_o"], 4, F, op)
        assert rc == C.MPI_ERR_TYPE and "no single basic element type" in err
        assert _both(L, 1, BF, 1, T["mixed_t"], op)[0] == C.MPI_ERR_TYPE
        # structs whose data bytes are no whole element of the kind asked for
        assert _both(L, 1, T["bytes2"], 1, F, op)[0] == C.MPI_ERR_TYPE
        assert _both(L, 1, BF, 1, T["bytes4"], op)[0] == C.MPI_ERR_TYPE


def test_every_fp32_handle_is_a_target_and_both_16_bit_types_an_origin(L, T):
    for tdt in (C.MPI_FLOAT, C.MPI_REAL, C.MPI_REAL4):
        for odt in (BF, HF):
            assert _plan(L, 8, odt, 8, tdt, C.MPI_PROD) == (0, 8, 1)
    assert _plan(L, 1, T["hv"], 1, T["fsub"], C.MPI_MAX) == (0, 15, 2)


def test_null_buffers_come_before_the_gpu(L, T):
    # check 7: on a host without a GPU check 8 is behind it
    for origin, target in ((None, BASE), (FAR, None), (None, None)):
        for a in ((1, T["bv"], 1, T["fsub"], C.MPI_SUM), (100, BF, 100, F, C.MPI_SUM), (100, HF, 100, F, C.MPI_REPLACE)):
            assert _plan(L, *a)[0] == 0
            assert L.msx_accumulate_widen_dev(origin, a[0], a[1], target, a[2], a[3], a[4], None) == C.MPI_ERR_BUFFER
            assert "null" in msx.last_error()


def test_valid_arguments_without_a_gpu_are_mpi_err_other_and_write_nothing(L, T):
    if L.msx_device_count() > 0:
        pytest.skip("GPU present")
    o = np.full(64, 0x3F80, np.uint16)
    t = np.full(64, 0x40400000, np.uint32)
    for a in ((64, BF, 64, F, C.MPI_SUM), (64, HF, 64, F, C.MPI_REPLACE), (1, T["bv"], 1, T["fsub"], C.MPI_MAX),
              (1, T["bix"], 1, T["fsub"], C.MPI_SUM)):
        assert _plan(L, *a)[0] == 0                   # the plan of the same arguments needs no GPU
        rc = L.msx_accumulate_widen_dev(o.ctypes.data, a[0], a[1], t.ctypes.data, a[2], a[3], a[4], None)
        assert rc == C.MPI_ERR_OTHER
        assert (t == 0x40400000).all() and (o == 0x3F80).all()


# ---- the plan's figures ------------------------------------------------------------

def test_plan_outputs_are_required(L, T):
    n, path = i64(), c_int()
    a = (1, T["bv"], 1, T["fsub"], C.MPI_SUM)
    assert L.msx_accumulate_widen_plan(*a, None, ctypes.byref(path)) == C.MPI_ERR_ARG
    assert L.msx_accumulate_widen_plan(*a, ctypes.byref(n), None) == C.MPI_ERR_ARG
    # before every other check
    assert L.msx_accumulate_widen_plan(-1, 0x1234, -1, 0x1234, 0x1234, None, None) == C.MPI_ERR_ARG


def test_plan_of_each_path(L, T):
    # 1: both pieces contiguous
    assert _plan(L, 100, BF, 100, F, C.MPI_SUM) == (0, 100, 1)
    assert _plan(L, 100, HF, 300, F, C.MPI_REPLACE) == (0, 100, 1)
    assert _plan(L, 10, T["bc10"], 10, T["fc10"], C.MPI_MAX) == (0, 100, 1)
    assert _plan(L, 3, BF, 1, T["fsub"], C.MPI_SUM) == (0, 3, 1)             # inside the target's first row of 5
    assert _plan(L, 1, BF, 1, T["fv3"], C.MPI_SUM) == (0, 1, 1)
    # 2: vector / contiguous, contiguous / subarray, indexed / subarray
    assert _plan(L, 1, T["bv"], 15, F, C.MPI_SUM) == (0, 15, 2)
    assert _plan(L, 2, T["bv"], 40, F, C.MPI_REPLACE) == (0, 30, 2)
    assert _plan(L, 15, BF, 1, T["fsub"], C.MPI_SUM) == (0, 15, 2)
    assert _plan(L, 6, BF, 1, T["fsub"], C.MPI_MIN) == (0, 6, 2)             # into the second row: partly covered
    assert _plan(L, 1, T["bix"], 1, T["fsub"], C.MPI_SUM) == (0, 14, 2)
    assert _plan(L, 2, T["bix"], 2, T["fsub"], C.MPI_PROD) == (0, 28, 2)
    assert _plan(L, 1, T["bv"], 1, T["fsub"], C.MPI_SUM) == (0, 15, 2)
    # 0: zero counts and MPI_NO_OP
    assert _plan(L, 0, T["bv"], 0, T["fsub"], C.MPI_SUM) == (0, 0, 0)
    assert _plan(L, 0, BF, 7, F, C.MPI_REPLACE) == (0, 0, 0)
    assert _plan(L, 1, T["bv"], 1, T["fsub"], C.MPI_NO_OP) == (0, 15, 0)


def test_msx_accumulate_dev_still_refuses_the_mixed_pair(L, T):
    """The widening call adds no pair to any existing one."""
    n, path, gran = i64(), c_int(), c_int()
    for op in (C.MPI_SUM, C.MPI_MAX):
        for odt, tdt in ((BF, F), (HF, F), (T["bv"], T["fsub"])):
            # 2 x the element count on the origin side, so the data bytes agree and check 6 is reached
            oc, tc = (8, 4) if odt in (BF, HF) else (2, 1)
            assert L.msx_accumulate_dev(None, oc, odt, None, tc, tdt, op, None) == C.MPI_ERR_TYPE
            assert "kind" in msx.last_error()
            assert L.msx_accumulate_plan(oc, odt, tc, tdt, op, ctypes.byref(n), ctypes.byref(path),
                                         ctypes.byref(gran)) == C.MPI_ERR_TYPE
