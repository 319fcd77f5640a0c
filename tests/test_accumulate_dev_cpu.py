"""CPU, no GPU: msx_accumulate_dev / msx_accumulate_plan (include/msx.h): the
two symbols, the order of the host-side checks and the plan's figures.

Every check-order case breaks one check and at least one later one; the class
that comes back names the check that ran first.  The plan is a pure function
of its arguments, so it runs without a GPU; the real call is driven only into
its checks (null or fake addresses are never dereferenced there) and, without
a GPU, to MPI_ERR_OTHER."""
import ctypes
import os
import re

import pytest

import msx
from test_dtype_cpu import build_lib, free_all

C = msx.C
vp, i64, c_int = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int

BASE = 0x7F0000000000          # a fake, 16-byte aligned device address
FAR = BASE + (1 << 36)


@pytest.fixture(scope="module")
def L():
    return msx.init(errors_return=True)


@pytest.fixture(scope="module")
def T(L):
    """Committed types by name, freed at the end; `raw` stays uncommitted."""
    keep = []
    f, b = ("basic", C.MPI_FLOAT), ("basic", C.MPI_BYTE)
    recipes = {
        "v5": ("vector", 37, 1, 5, f),                    # 37 floats, one per 20 bytes
        "v3": ("vector", 37, 1, 3, f),
        "v2x60": ("vector", 60, 1, 2, f),
        "c10": ("contig", 10, f),
        "vi3": ("vector", 37, 1, 3, ("basic", C.MPI_INT)),
        "vfi": ("vector", 4, 1, 2, ("basic", C.MPI_FLOAT_INT)),
        "mixed": ("struct", [1, 1], [0, 8], [("basic", C.MPI_INT8_T), ("basic", C.MPI_DOUBLE)]),
        "b16": ("vector", 37, 16, 48, b),
        "b2": ("vector", 37, 2, 6, b),
        "b1": ("vector", 37, 1, 3, b),
        "ix": ("indexed", [3, 1, 4, 1, 5], [0, 5, 7, 13, 16], f),
        "sub": ("subarray", [6, 7, 8], [3, 4, 5], [2, 1, 3], True, f),
    }
    out = {}
    for name, r in recipes.items():
        h = build_lib(L, r, keep)
        x = c_int(h)
        assert L.MPI_Type_commit(ctypes.byref(x)) == 0
        out[name] = h
    out["raw"] = build_lib(L, ("vector", 3, 1, 2, f), keep)
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
    """(rc, elements, path, granule)"""
    n, path, gran = i64(-7), c_int(-7), c_int(-7)
    rc = L.msx_accumulate_plan(oc, odt, tc, tdt, op, ctypes.byref(n), ctypes.byref(path), ctypes.byref(gran))
    return rc, n.value, path.value, gran.value


def _both(L, oc, odt, tc, tdt, op, origin=None, target=None):
    """The class both entry points return for arguments that fail a check."""
    rc = L.msx_accumulate_dev(origin, oc, odt, target, tc, tdt, op, None)
    err = msx.last_error()
    assert rc != 0
    assert _plan(L, oc, odt, tc, tdt, op)[0] == rc
    return rc, err


# ---- the symbols -------------------------------------------------------------------

def test_both_symbols_are_exported_and_declared(L):
    with open(os.path.join(msx.INCLUDE_DIR, "msx.h")) as f:
        txt = f.read()
    for name in ("msx_accumulate_dev", "msx_accumulate_plan"):
        assert hasattr(L, name)
        assert name in msx.exported_symbols()
        assert re.search(r"^int %s\(" % name, txt, re.M)


# ---- the order of the checks -------------------------------------------------------

def test_counts_come_first(L, T):
    # check 1, with a bad datatype, a bad op, truncation and null buffers behind it
    for oc, tc in ((-1, 1), (1, -1), (-5, -5)):
        assert _both(L, oc, 0x1234, tc, T["raw"], 0x1234)[0] == C.MPI_ERR_COUNT
        assert _both(L, oc, T["v5"], tc, T["v3"], C.MPI_SUM)[0] == C.MPI_ERR_COUNT


def test_datatypes_come_before_the_op(L, T, user_op):
    # check 2, with a bad op, truncation, unlike element kinds and null buffers behind it
    for op in (0x1234, user_op, C.MSX_SUM_WIDE, C.MPI_SUM):
        assert _both(L, 9, 0x1234, 1, T["vi3"], op)[0] == C.MPI_ERR_TYPE
        assert _both(L, 9, T["v5"], 1, C.MPI_DATATYPE_NULL, op)[0] == C.MPI_ERR_TYPE
        rc, err = _both(L, 9, T["raw"], 1, T["vi3"], op)
        assert rc == C.MPI_ERR_TYPE and "not committed" in err
        rc, err = _both(L, 9, T["v5"], 1, T["raw"], op)
        assert rc == C.MPI_ERR_TYPE and "not committed" in err


def test_the_op_comes_before_truncation_and_the_element_types(L, T, user_op, device_op):
    # check 3: 9 x 37 floats into 1 x 37 ints behind it (truncation, unlike kinds, null buffers)
    a = (9, T["v5"], 1, T["vi3"])
    assert _both(L, *a, 0x1234)[0] == C.MPI_ERR_OP
    assert _both(L, *a, C.MPI_OP_NULL)[0] == C.MPI_ERR_OP
    rc, err = _both(L, *a, user_op)
    assert rc == C.MPI_ERR_OP and "builtin ops only" in err
    rc, err = _both(L, *a, device_op)
    assert rc == C.MPI_ERR_OP and "builtin ops only" in err
    rc, err = _both(L, *a, C.MSX_SUM_WIDE)
    assert rc == C.MPI_ERR_OP and "MSX_SUM_WIDE" in err
    # also on the 16-bit floats, where MSX_SUM_WIDE is legal elsewhere
    rc, err = _both(L, 4, C.MSX_BFLOAT16, 4, C.MSX_BFLOAT16, C.MSX_SUM_WIDE)
    assert rc == C.MPI_ERR_OP and "MSX_SUM_WIDE" in err


def test_truncation_comes_before_the_element_types(L, T):
    # check 4: unlike kinds, an illegal pair and null buffers behind it
    for op in (C.MPI_SUM, C.MPI_BAND, C.MPI_REPLACE):
        rc, err = _both(L, 2, T["v5"], 1, T["vi3"], op)
        assert rc == C.MPI_ERR_TRUNCATE and "296" in err and "148" in err
    assert _both(L, 1, T["v5"], 0, T["vi3"], C.MPI_SUM)[0] == C.MPI_ERR_TRUNCATE
    assert _both(L, 1, C.MPI_DOUBLE, 1, C.MPI_FLOAT, C.MPI_SUM)[0] == C.MPI_ERR_TRUNCATE
    # MPI_NO_OP is looked at after the sizes
    assert _both(L, 2, T["v5"], 1, T["v3"], C.MPI_NO_OP)[0] == C.MPI_ERR_TRUNCATE


def test_nothing_to_do_succeeds_before_the_element_types_and_the_buffers(L, T):
    # check 5: unlike kinds, an illegal pair, a type without an element type, null buffers
    for odt, tdt, op in ((T["v5"], T["vi3"], C.MPI_SUM), (T["v5"], T["v3"], C.MPI_BAND),
                         (T["vfi"], T["mixed"], C.MPI_MAXLOC)):
        assert L.msx_accumulate_dev(None, 0, odt, None, 3, tdt, op, None) == 0
        assert L.msx_accumulate_dev(None, 0, odt, None, 0, tdt, op, None) == 0
        assert _plan(L, 0, odt, 3, tdt, op) == (0, 0, 0, 0)
    assert L.msx_accumulate_dev(None, 1, T["mixed"], None, 2, T["v5"], C.MPI_NO_OP, None) == 0
    assert L.msx_accumulate_dev(None, 1, T["v5"], None, 1, T["vi3"], C.MPI_NO_OP, None) == 0
    assert _plan(L, 1, T["v5"], 1, T["vi3"], C.MPI_NO_OP) == (0, 37, 0, 0)
    assert _plan(L, 3, T["mixed"], 1, T["v5"], C.MPI_NO_OP) == (0, 6, 0, 0)


def test_element_types_come_before_the_buffers(L, T):
    # check 6 with null buffers behind it; inside it the types come before the pair
    rc, err = _both(L, 1, T["v5"], 1, T["vi3"], C.MPI_SUM)
    assert rc == C.MPI_ERR_TYPE and "kind" in err
    assert _both(L, 1, T["v5"], 1, T["vi3"], C.MPI_BAND)[0] == C.MPI_ERR_TYPE       # BAND on floats behind it
    rc, err = _both(L, 1, T["vfi"], 1, T["vfi"], C.MPI_MAXLOC)
    assert rc == C.MPI_ERR_TYPE and "no single basic element type" in err
    assert _both(L, 1, T["mixed"], 1, T["mixed"], C.MPI_SUM)[0] == C.MPI_ERR_TYPE
    assert _both(L, 4, C.MPI_FLOAT, 1, T["vfi"], C.MPI_SUM)[0] == C.MPI_ERR_TYPE
    rc, err = _both(L, 1, T["v5"], 1, T["v3"], C.MPI_BAND)
    assert rc == C.MPI_ERR_OP and "MPI_BAND" in err
    assert _both(L, 1, T["v5"], 1, T["v3"], C.MPI_MAXLOC)[0] == C.MPI_ERR_OP
    assert _both(L, 1, T["b1"], 1, T["b1"], C.MPI_SUM)[0] == C.MPI_ERR_OP           # MPI_BYTE: bit ops only
    assert _both(L, 4, C.MSX_FLOAT16, 4, C.MSX_FLOAT16, C.MPI_LAND)[0] == C.MPI_ERR_OP
    # MPI_REPLACE asks nothing of the element types: these reach the buffer check
    for odt, tdt in ((T["v5"], T["vi3"]), (T["mixed"], T["b16"]), (T["vfi"], T["v5"])):
        rc, err = _both_buffers(L, 1, odt, 3, tdt, C.MPI_REPLACE)
        assert rc == C.MPI_ERR_BUFFER and "null" in err


def _both_buffers(L, oc, odt, tc, tdt, op):
    """The real call with null buffers; the plan of the same arguments passes."""
    assert _plan(L, oc, odt, tc, tdt, op)[0] == 0
    rc = L.msx_accumulate_dev(None, oc, odt, None, tc, tdt, op, None)
    return rc, msx.last_error()


def test_null_buffers_come_before_the_gpu(L, T):
    # check 7: on a host without a GPU check 8 is behind it
    for origin, target in ((None, BASE), (FAR, None), (None, None)):
        for a in ((1, T["v5"], 1, T["v3"], C.MPI_SUM), (100, C.MPI_FLOAT, 100, C.MPI_FLOAT, C.MPI_SUM),
                  (1, T["b2"], 1, T["b16"], C.MPI_REPLACE)):
            assert _plan(L, *a)[0] == 0
            assert L.msx_accumulate_dev(origin, a[0], a[1], target, a[2], a[3], a[4], None) == C.MPI_ERR_BUFFER
            assert "null" in msx.last_error()


def test_valid_arguments_without_a_gpu_are_mpi_err_other(L, T):
    if L.msx_device_count() > 0:
        pytest.skip("GPU present")
    for a in ((1, T["v5"], 1, T["v3"], C.MPI_SUM), (100, C.MPI_FLOAT, 100, C.MPI_FLOAT, C.MPI_MAX),
              (111, C.MPI_FLOAT, 3, T["v3"], C.MPI_SUM), (1, T["v5"], 37, C.MPI_FLOAT, C.MPI_REPLACE),
              (1, T["ix"], 1, T["b16"], C.MPI_REPLACE)):
        assert L.msx_accumulate_dev(FAR, a[0], a[1], BASE, a[2], a[3], a[4], None) == C.MPI_ERR_OTHER
        assert _plan(L, *a)[0] == 0               # and the plan of the same arguments needs none


# ---- the plan's figures ------------------------------------------------------------

def test_plan_outputs_are_required(L, T):
    n, path, gran = i64(), c_int(), c_int()
    a = (1, T["v5"], 1, T["v3"], C.MPI_SUM)
    assert L.msx_accumulate_plan(*a, None, ctypes.byref(path), ctypes.byref(gran)) == C.MPI_ERR_ARG
    assert L.msx_accumulate_plan(*a, ctypes.byref(n), None, ctypes.byref(gran)) == C.MPI_ERR_ARG
    assert L.msx_accumulate_plan(*a, ctypes.byref(n), ctypes.byref(path), None) == C.MPI_ERR_ARG
    # before every other check
    assert L.msx_accumulate_plan(-1, 0x1234, -1, 0x1234, 0x1234, None, None, None) == C.MPI_ERR_ARG


def test_plan_of_each_path(L, T):
    F = C.MPI_FLOAT
    # 1: both sides in one piece
    assert _plan(L, 100, F, 100, F, C.MPI_SUM) == (0, 100, 1, 4)
    assert _plan(L, 10, T["c10"], 200, F, C.MPI_MAX) == (0, 100, 1, 4)
    assert _plan(L, 100, F, 10, T["c10"], C.MPI_REPLACE) == (0, 100, 1, 4)
    assert _plan(L, 1, F, 1, T["v3"], C.MPI_SUM) == (0, 1, 1, 4)            # one element of a strided target
    # 2: the origin in one piece over whole target instances
    assert _plan(L, 111, F, 3, T["v3"], C.MPI_SUM) == (0, 111, 2, 4)
    assert _plan(L, 37, F, 3, T["v3"], C.MPI_REPLACE) == (0, 37, 2, 4)
    assert _plan(L, 4, T["c10"], 1, T["v2x60"], C.MPI_SUM)[2] == 4           # 40 of 60 elements: the two-layout kernel
    # 3: a copy into one piece
    assert _plan(L, 1, T["v5"], 37, F, C.MPI_REPLACE) == (0, 37, 3, 4)
    assert _plan(L, 1, T["v5"], 37, F, C.MPI_SUM) == (0, 37, 4, 4)           # no existing kernel combines that way
    # 4: a layout on both sides
    assert _plan(L, 1, T["v5"], 1, T["v3"], C.MPI_SUM) == (0, 37, 4, 4)
    assert _plan(L, 3, T["v5"], 3, T["v3"], C.MPI_REPLACE) == (0, 111, 4, 4)
    assert _plan(L, 2, T["ix"], 1, T["v3"], C.MPI_MIN) == (0, 28, 4, 4)
    assert _plan(L, 1, T["ix"], 1, T["ix"], C.MPI_PROD) == (0, 14, 4, 4)
    # a subarray's MPI_LB / MPI_UB markers are no elements
    assert _plan(L, 2, T["sub"], 120, F, C.MPI_REPLACE) == (0, 120, 3, 4)
    assert _plan(L, 2, T["sub"], 4, T["v3"], C.MPI_SUM) == (0, 120, 4, 4)


def test_plan_granule(L, T):
    # an op: the element size, whatever the layouts would allow
    for dt, esz in ((C.MPI_INT8_T, 1), (C.MSX_FLOAT16, 2), (C.MPI_DOUBLE, 8), (C.MPI_C_DOUBLE_COMPLEX, 16),
                    (C.MPI_2INT, 8)):
        assert _plan(L, 10, dt, 10, dt, C.MPI_MAXLOC if dt == C.MPI_2INT else C.MPI_SUM) == (0, 10, 1, esz)
    # MPI_REPLACE: the largest power of two <= 16 common to both layouts
    assert _plan(L, 1, T["b16"], 1, T["b16"], C.MPI_REPLACE) == (0, 592, 4, 16)
    assert _plan(L, 1, T["b2"], 8, T["b16"], C.MPI_REPLACE) == (0, 74, 4, 2)
    assert _plan(L, 1, T["b16"], 592, T["b1"], C.MPI_REPLACE)[2:] == (4, 1)
    assert _plan(L, 4, T["v5"], 1, T["b16"], C.MPI_REPLACE) == (0, 148, 4, 4)
    # a mixed struct (int8 at 0, double at 8: runs of 1 and 8 bytes) copies byte by byte
    assert _plan(L, 2, T["mixed"], 1, T["b16"], C.MPI_REPLACE) == (0, 4, 4, 1)
