"""CPU, no GPU: msx_fetch_and_op_dev, msx_get_accumulate_dev and
msx_get_accumulate_plan (include/msx.h): the three symbols, the order of the
host-side checks and the plan's figures.

Every check-order case breaks one check and at least one later one; the class
(and, where several checks share a class, the text) that comes back names the
check that ran first.  The plan is a pure function of its arguments, so it runs
without a GPU; the real calls are driven only into their checks (null or fake
addresses are never dereferenced there) and, without a GPU, to MPI_ERR_OTHER.
No case here hands fake addresses to a call that could reach a launch on a host
that has a GPU."""
import ctypes
import os
import re
import subprocess
import sys
import textwrap

import pytest

import msx
from test_dtype_cpu import build_lib, free_all

C = msx.C
vp, i64, c_int = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int

BASE = 0x7F0000000000          # fake, 16-byte aligned device addresses, 2^36 apart
FAR = BASE + (1 << 36)
FAR2 = BASE + (2 << 36)


@pytest.fixture(scope="module")
def L():
    return msx.init(errors_return=True)


@pytest.fixture(scope="module")
def T(L):
    """Committed types by name, freed at the end; `raw` stays uncommitted."""
    keep = []
    f, b = ("basic", C.MPI_FLOAT), ("basic", C.MPI_BYTE)
    recipes = {
        "v16": ("vector", 37, 4, 8, f),                   # 16-byte blocks at a 32-byte stride, 148 floats
        "v5": ("vector", 37, 1, 5, f),
        "v3": ("vector", 37, 1, 3, f),
        "v6x5": ("vector", 5, 4, 6, f),                   # a first run of 16 bytes
        "c10": ("contig", 10, f),
        "vi3": ("vector", 37, 1, 3, ("basic", C.MPI_INT)),
        "vfi": ("vector", 4, 1, 2, ("basic", C.MPI_FLOAT_INT)),
        "mixed": ("struct", [1, 1], [0, 8], [("basic", C.MPI_INT8_T), ("basic", C.MPI_DOUBLE)]),
        "b1": ("vector", 37, 1, 3, b),
        "b2": ("vector", 37, 2, 6, b),
        "ix": ("indexed", [3, 1, 4, 1, 5], [0, 5, 7, 13, 16], f),          # 14 floats in 5 uneven runs
        "sub": ("subarray", [6, 7, 8], [3, 4, 5], [2, 1, 3], True, f),      # 60 floats in rows of 5
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


def _plan(L, oc, odt, rc_, rdt, tc, tdt, op):
    """(rc, elements, path, granule)"""
    n, path, gran = i64(-7), c_int(-7), c_int(-7)
    rc = L.msx_get_accumulate_plan(oc, odt, rc_, rdt, tc, tdt, op, ctypes.byref(n), ctypes.byref(path),
                                   ctypes.byref(gran))
    return rc, n.value, path.value, gran.value


def _both(L, a, op, origin=None, result=None, target=None):
    """The class both entry points return for a = (oc, odt, rc, rdt, tc, tdt)
    failing one of checks 1 - 6."""
    rc = L.msx_get_accumulate_dev(origin, a[0], a[1], result, a[2], a[3], target, a[4], a[5], op, None)
    err = msx.last_error()
    assert rc != 0
    assert _plan(L, *a, op)[0] == rc
    return rc, err


def _fop(L, in_, fetched, inout, count, dt, op):
    rc = L.msx_fetch_and_op_dev(in_, fetched, inout, count, dt, op, None)
    return rc, msx.last_error()


# ---- the symbols -------------------------------------------------------------------

def test_the_symbols_are_exported_and_declared(L):
    with open(os.path.join(msx.INCLUDE_DIR, "msx.h")) as f:
        txt = f.read()
    for name in ("msx_fetch_and_op_dev", "msx_get_accumulate_dev", "msx_get_accumulate_plan"):
        assert hasattr(L, name)
        assert name in msx.exported_symbols()
        assert re.search(r"^int %s\(" % name, txt, re.M)


# ---- msx_fetch_and_op_dev: the order of the checks ---------------------------------

def test_fetch_count_zero_succeeds_before_everything(L, user_op):
    # check 1, with a bad op, an illegal pair and null buffers behind it
    for dt, op in ((0x1234, 0x1234), (C.MPI_FLOAT, user_op), (C.MPI_FLOAT, C.MPI_BAND), (C.MPI_FLOAT, C.MPI_SUM)):
        assert L.msx_fetch_and_op_dev(None, None, None, 0, dt, op, None) == 0


def test_fetch_op_comes_before_the_count_and_the_buffers(L, user_op, device_op):
    # check 2, with a negative count, null buffers and aliasing behind it
    for count, bufs in ((-1, (None, None, None)), (5, (BASE, BASE, BASE))):
        assert _fop(L, *bufs, count, C.MPI_FLOAT, 0x1234)[0] == C.MPI_ERR_OP
        assert _fop(L, *bufs, count, C.MPI_FLOAT, C.MPI_OP_NULL)[0] == C.MPI_ERR_OP
        for op in (user_op, device_op):
            rc, err = _fop(L, *bufs, count, C.MPI_FLOAT, op)
            assert rc == C.MPI_ERR_OP and "builtin ops only" in err
        for dt, op in ((C.MPI_FLOAT, C.MPI_BAND), (C.MPI_FLOAT, C.MPI_MAXLOC), (C.MPI_FLOAT_INT, C.MPI_SUM),
                       (C.MPI_BYTE, C.MPI_SUM), (C.MSX_FLOAT16, C.MPI_LAND), (C.MPI_FLOAT, C.MSX_SUM_WIDE),
                       (0x1234, C.MPI_SUM), (C.MPI_DATATYPE_NULL, C.MPI_MAX)):
            rc, err = _fop(L, *bufs, count, dt, op)
            assert rc == C.MPI_ERR_OP and "not defined" in err, (dt, op, err)
        # MPI_REPLACE / MPI_NO_OP take predefined datatypes that hold data
        for dt in (0x1234, C.MPI_DATATYPE_NULL, C.MPI_LB):
            for op in (C.MPI_REPLACE, C.MPI_NO_OP):
                assert _fop(L, *bufs, count, dt, op)[0] == C.MPI_ERR_OP


def test_fetch_derived_datatypes_are_refused_with_the_op(L, T):
    for op in (C.MPI_SUM, C.MPI_REPLACE, C.MPI_NO_OP):
        assert _fop(L, None, None, None, -1, T["c10"], op)[0] == C.MPI_ERR_OP


def test_fetch_negative_count_comes_before_the_buffers(L):
    # check 3, with null buffers and aliasing behind it
    for op, dt in ((C.MPI_SUM, C.MPI_FLOAT), (C.MPI_MAXLOC, C.MPI_DOUBLE_INT), (C.MSX_SUM_WIDE, C.MSX_BFLOAT16),
                   (C.MPI_REPLACE, C.MPI_WCHAR), (C.MPI_NO_OP, C.MPI_FLOAT)):
        assert _fop(L, None, None, None, -3, dt, op)[0] == C.MPI_ERR_COUNT
        assert _fop(L, BASE, BASE, BASE, -3, dt, op)[0] == C.MPI_ERR_COUNT
    assert _fop(L, BASE, FAR, FAR2, 1 << 62, C.MPI_DOUBLE, C.MPI_SUM)[0] == C.MPI_ERR_COUNT


def test_fetch_null_buffers_come_before_the_aliasing(L):
    # check 4: the non-null operands alias each other (checks 5 and 6 behind it)
    for in_, fetched, inout in ((None, BASE, BASE), (BASE, None, BASE), (BASE, BASE, None), (None, None, None)):
        rc, err = _fop(L, in_, fetched, inout, 8, C.MPI_FLOAT, C.MPI_SUM)
        assert rc == C.MPI_ERR_BUFFER and "null" in err
        rc, err = _fop(L, in_, fetched, inout, 8, C.MPI_FLOAT, C.MPI_REPLACE)
        assert rc == C.MPI_ERR_BUFFER and "null" in err
    # MPI_NO_OP never looks at `in`, but needs the other two
    for fetched, inout in ((None, BASE), (BASE, None)):
        rc, err = _fop(L, None, fetched, inout, 8, C.MPI_FLOAT, C.MPI_NO_OP)
        assert rc == C.MPI_ERR_BUFFER and "null" in err


def test_fetch_in_equal_to_inout_comes_before_the_ranges(L):
    # check 5, with fetched inside both behind it
    rc, err = _fop(L, BASE, BASE + 16, BASE, 100, C.MPI_FLOAT, C.MPI_SUM)
    assert rc == C.MPI_ERR_BUFFER and "aliases" in err
    rc, err = _fop(L, BASE, FAR, BASE, 100, C.MPI_FLOAT, C.MPI_REPLACE)
    assert rc == C.MPI_ERR_BUFFER and "aliases" in err


def test_fetch_ranges_that_meet_are_refused_and_named(L):
    # check 6: 100 floats are 400 bytes
    for fetched in (BASE, BASE + 396, BASE - 396, BASE + 4):
        rc, err = _fop(L, FAR, fetched, BASE, 100, C.MPI_FLOAT, C.MPI_SUM)
        assert rc == C.MPI_ERR_BUFFER and "fetched" in err and "inout" in err, err
        rc, err = _fop(L, BASE, fetched, FAR, 100, C.MPI_FLOAT, C.MPI_MAX)
        assert rc == C.MPI_ERR_BUFFER and "fetched" in err and re.search(r"\bin\b", err), err
    # the range is count x the struct size for a pair type
    rc, err = _fop(L, FAR, BASE + 1599, BASE, 100, C.MPI_DOUBLE_INT, C.MPI_MAXLOC)
    assert rc == C.MPI_ERR_BUFFER and "inout" in err
    # MPI_NO_OP: fetched against inout only (`in` is not an operand)
    rc, err = _fop(L, None, BASE + 8, BASE, 100, C.MPI_FLOAT, C.MPI_NO_OP)
    assert rc == C.MPI_ERR_BUFFER and "inout" in err


def test_fetch_valid_arguments_without_a_gpu_are_mpi_err_other(L):
    if L.msx_device_count() > 0:
        pytest.skip("GPU present")
    for dt, op in ((C.MPI_FLOAT, C.MPI_SUM), (C.MPI_DOUBLE_INT, C.MPI_MINLOC), (C.MSX_FLOAT16, C.MSX_SUM_WIDE),
                   (C.MPI_WCHAR, C.MPI_REPLACE)):
        assert _fop(L, BASE, FAR, FAR2, 100, dt, op)[0] == C.MPI_ERR_OTHER
        # ranges that touch end to start do not meet
        assert _fop(L, BASE, BASE + 100 * msx.lib().msx_type_size(dt), FAR, 100, dt, op)[0] == C.MPI_ERR_OTHER
    assert _fop(L, None, FAR, FAR2, 100, C.MPI_FLOAT, C.MPI_NO_OP)[0] == C.MPI_ERR_OTHER
    assert _fop(L, FAR2, FAR, FAR2, 100, C.MPI_FLOAT, C.MPI_NO_OP)[0] == C.MPI_ERR_OTHER     # `in` is not looked at


# ---- msx_get_accumulate_dev: the order of the checks -------------------------------

def test_counts_come_first(L, T):
    # check 1, with a bad datatype, a bad op, truncation and null buffers behind it
    for oc, rc_, tc in ((-1, 1, 1), (1, -1, 1), (1, 1, -1), (-5, -5, -5)):
        assert _both(L, (oc, 0x1234, rc_, T["raw"], tc, 0x1234), 0x1234)[0] == C.MPI_ERR_COUNT
        assert _both(L, (oc, T["v5"], rc_, T["v3"], tc, T["v3"]), C.MPI_SUM)[0] == C.MPI_ERR_COUNT
    # MPI_NO_OP ignores the origin's count, not the other two
    assert _both(L, (-1, T["v5"], -1, T["v3"], 1, T["v3"]), C.MPI_NO_OP)[0] == C.MPI_ERR_COUNT
    assert _both(L, (-1, T["v5"], 1, T["v3"], -1, T["v3"]), C.MPI_NO_OP)[0] == C.MPI_ERR_COUNT


def test_datatypes_come_before_the_op(L, T, user_op):
    # check 2, with a bad op, truncation, unlike element kinds and null buffers behind it
    for op in (0x1234, user_op, C.MSX_SUM_WIDE, C.MPI_SUM):
        for bad in (0x1234, C.MPI_DATATYPE_NULL):
            assert _both(L, (9, bad, 1, T["vi3"], 1, T["v3"]), op)[0] == C.MPI_ERR_TYPE
            assert _both(L, (9, T["v5"], 1, bad, 1, T["v3"]), op)[0] == C.MPI_ERR_TYPE
            assert _both(L, (9, T["v5"], 1, T["vi3"], 1, bad), op)[0] == C.MPI_ERR_TYPE
        for k in range(3):
            a = [9, T["v5"], 1, T["vi3"], 1, T["v3"]]
            a[2 * k + 1] = T["raw"]
            rc, err = _both(L, tuple(a), op)
            assert rc == C.MPI_ERR_TYPE and "not committed" in err
    # under MPI_NO_OP the origin's datatype is not looked at; the other two are
    assert _both(L, (1, 0x1234, 1, 0x1234, 1, T["v3"]), C.MPI_NO_OP)[0] == C.MPI_ERR_TYPE
    assert _both(L, (1, 0x1234, 1, T["v3"], 1, T["raw"]), C.MPI_NO_OP)[0] == C.MPI_ERR_TYPE


def test_the_op_comes_before_truncation_and_the_element_types(L, T, user_op, device_op):
    # check 3: 9 x 37 floats into 1 x 37 ints behind it (truncation, unlike kinds, null buffers)
    a = (9, T["v5"], 1, T["vi3"], 1, T["vi3"])
    assert _both(L, a, 0x1234)[0] == C.MPI_ERR_OP
    assert _both(L, a, C.MPI_OP_NULL)[0] == C.MPI_ERR_OP
    for op in (user_op, device_op):
        rc, err = _both(L, a, op)
        assert rc == C.MPI_ERR_OP and "builtin ops only" in err
    rc, err = _both(L, a, C.MSX_SUM_WIDE)
    assert rc == C.MPI_ERR_OP and "MSX_SUM_WIDE" in err
    rc, err = _both(L, (4, C.MSX_BFLOAT16, 4, C.MSX_BFLOAT16, 4, C.MSX_BFLOAT16), C.MSX_SUM_WIDE)
    assert rc == C.MPI_ERR_OP and "MSX_SUM_WIDE" in err


def test_truncation_against_the_target_and_against_the_result(L, T):
    # check 4: unlike kinds, an illegal pair and null buffers behind it.  2 x 37 floats are 296 bytes.
    for op in (C.MPI_SUM, C.MPI_BAND, C.MPI_REPLACE):
        rc, err = _both(L, (2, T["v5"], 2, T["vi3"], 1, T["vi3"]), op)            # the target is short
        assert rc == C.MPI_ERR_TRUNCATE and "296" in err and "148" in err and "result" not in err
        rc, err = _both(L, (2, T["v5"], 1, T["vi3"], 2, T["vi3"]), op)            # the result is short
        assert rc == C.MPI_ERR_TRUNCATE and "296" in err and "148" in err and "result" in err
    assert _both(L, (1, T["v5"], 1, T["v3"], 0, T["v3"]), C.MPI_SUM)[0] == C.MPI_ERR_TRUNCATE
    assert _both(L, (1, T["v5"], 0, T["v3"], 1, T["v3"]), C.MPI_SUM)[0] == C.MPI_ERR_TRUNCATE
    assert _both(L, (1, C.MPI_DOUBLE, 2, C.MPI_FLOAT, 1, C.MPI_FLOAT), C.MPI_SUM)[0] == C.MPI_ERR_TRUNCATE
    # MPI_NO_OP: the result triple's bytes against the target's
    assert _both(L, (0, 0x1234, 2, T["v5"], 1, T["v3"]), C.MPI_NO_OP)[0] == C.MPI_ERR_TRUNCATE
    # sizes beyond 2^62
    big = 1 << 61
    assert _both(L, (big, C.MPI_DOUBLE, big, C.MPI_DOUBLE, big, C.MPI_DOUBLE), C.MPI_SUM)[0] == C.MPI_ERR_COUNT
    assert _both(L, (1, C.MPI_FLOAT, 1, C.MPI_FLOAT, big, T["vi3"]), C.MPI_SUM)[0] == C.MPI_ERR_COUNT


def test_nothing_to_do_succeeds_before_the_element_types_and_the_buffers(L, T):
    # check 5: unlike kinds, an illegal pair, a type without an element type, null buffers
    for odt, rdt, tdt, op in ((T["v5"], T["vi3"], T["v3"], C.MPI_SUM), (T["v5"], T["v3"], T["v3"], C.MPI_BAND),
                              (T["vfi"], T["mixed"], T["mixed"], C.MPI_MAXLOC)):
        for rc_, tc in ((3, 3), (0, 0)):
            assert L.msx_get_accumulate_dev(None, 0, odt, None, rc_, rdt, None, tc, tdt, op, None) == 0
            assert _plan(L, 0, odt, rc_, rdt, tc, tdt, op) == (0, 0, 0, 0)
    # MPI_NO_OP with an empty result triple, whatever the origin says
    assert L.msx_get_accumulate_dev(None, 7, T["v5"], None, 0, T["v3"], None, 2, T["mixed"], C.MPI_NO_OP, None) == 0
    assert _plan(L, 7, T["v5"], 0, T["v3"], 2, T["mixed"], C.MPI_NO_OP) == (0, 0, 0, 0)


def test_element_types_come_before_the_buffers(L, T):
    # check 6 with null buffers behind it; inside it the types come before the pair
    rc, err = _both(L, (1, T["v5"], 1, T["v3"], 1, T["vi3"]), C.MPI_SUM)
    assert rc == C.MPI_ERR_TYPE and "kind" in err and "origin" in err
    rc, err = _both(L, (1, T["v5"], 1, T["vi3"], 1, T["v3"]), C.MPI_SUM)
    assert rc == C.MPI_ERR_TYPE and "kind" in err and "result" in err
    assert _both(L, (1, T["v5"], 1, T["vi3"], 1, T["v3"]), C.MPI_BAND)[0] == C.MPI_ERR_TYPE   # BAND on floats behind it
    for k, name in enumerate(("origin", "result", "target")):
        a = [1, T["v5"], 1, T["v3"], 1, T["v3"]]
        a[2 * k + 1] = T["mixed"]
        a[2 * k] = 37 if k else 1                  # 9 data bytes each: no truncation either way
        rc, err = _both(L, tuple(a), C.MPI_SUM)
        assert rc == C.MPI_ERR_TYPE and "no single basic element type" in err and name in err, err
    assert _both(L, (1, T["vfi"], 1, T["vfi"], 1, T["vfi"]), C.MPI_MAXLOC)[0] == C.MPI_ERR_TYPE
    rc, err = _both(L, (1, T["v5"], 1, T["v3"], 1, T["v3"]), C.MPI_BAND)
    assert rc == C.MPI_ERR_OP and "MPI_BAND" in err
    assert _both(L, (1, T["v5"], 1, T["v3"], 1, T["v3"]), C.MPI_MAXLOC)[0] == C.MPI_ERR_OP
    assert _both(L, (1, T["b1"], 1, T["b1"], 1, T["b1"]), C.MPI_SUM)[0] == C.MPI_ERR_OP       # MPI_BYTE: bit ops only
    assert _both(L, (4, C.MSX_FLOAT16, 4, C.MSX_FLOAT16, 4, C.MSX_FLOAT16), C.MPI_LAND)[0] == C.MPI_ERR_OP
    # MPI_REPLACE and MPI_NO_OP ask nothing of the element types: these reach the buffer check
    for a in ((1, T["v5"], 1, T["vi3"], 1, T["vi3"]), (4, T["mixed"], 1, T["b2"], 3, T["vfi"])):
        for op in (C.MPI_REPLACE, C.MPI_NO_OP):
            assert _plan(L, *a, op)[0] == 0, msx.last_error()
            assert L.msx_get_accumulate_dev(None, a[0], a[1], None, a[2], a[3], None, a[4], a[5], op, None) \
                == C.MPI_ERR_BUFFER
            assert "null" in msx.last_error()


def test_null_buffers_come_before_the_gpu(L, T):
    # check 7: on a host without a GPU check 8 is behind it
    cases = ((1, T["v5"], 1, T["v3"], 1, T["v16"], C.MPI_SUM), (100, C.MPI_FLOAT, 100, C.MPI_FLOAT, 100, C.MPI_FLOAT, C.MPI_SUM),
             (1, T["b2"], 1, T["b2"], 1, T["b2"], C.MPI_REPLACE))
    for origin, result, target in ((None, FAR, BASE), (FAR2, None, BASE), (FAR2, FAR, None), (None, None, None)):
        for a in cases:
            assert _plan(L, *a)[0] == 0
            rc = L.msx_get_accumulate_dev(origin, a[0], a[1], result, a[2], a[3], target, a[4], a[5], a[6], None)
            assert rc == C.MPI_ERR_BUFFER and "null" in msx.last_error()
    # MPI_NO_OP may leave the origin out, not the other two
    for result, target in ((None, BASE), (FAR, None)):
        rc = L.msx_get_accumulate_dev(None, 0, 0x1234, result, 1, T["v3"], target, 1, T["v3"], C.MPI_NO_OP, None)
        assert rc == C.MPI_ERR_BUFFER and "null" in msx.last_error()


def test_valid_arguments_without_a_gpu_are_mpi_err_other(L, T):
    if L.msx_device_count() > 0:
        pytest.skip("GPU present")
    for a in ((1, T["v5"], 1, T["v3"], 1, T["v16"], C.MPI_SUM), (100, C.MPI_FLOAT, 100, C.MPI_FLOAT, 100, C.MPI_FLOAT, C.MPI_MAX),
              (1, T["ix"], 1, T["b2"], 1, T["sub"], C.MPI_REPLACE), (-1, 0x1234, 1, T["v3"], 1, T["v5"], C.MPI_NO_OP)):
        origin = None if a[6] == C.MPI_NO_OP else FAR2
        rc = L.msx_get_accumulate_dev(origin, a[0], a[1], FAR, a[2], a[3], BASE, a[4], a[5], a[6], None)
        assert rc == C.MPI_ERR_OTHER
        assert _plan(L, *a)[0] == 0               # and the plan of the same arguments needs none


# ---- the plan's figures ------------------------------------------------------------

def test_plan_outputs_are_required(L, T):
    n, path, gran = i64(), c_int(), c_int()
    a = (1, T["v5"], 1, T["v3"], 1, T["v3"], C.MPI_SUM)
    assert L.msx_get_accumulate_plan(*a, None, ctypes.byref(path), ctypes.byref(gran)) == C.MPI_ERR_ARG
    assert L.msx_get_accumulate_plan(*a, ctypes.byref(n), None, ctypes.byref(gran)) == C.MPI_ERR_ARG
    assert L.msx_get_accumulate_plan(*a, ctypes.byref(n), ctypes.byref(path), None) == C.MPI_ERR_ARG
    # before every other check
    assert L.msx_get_accumulate_plan(-1, 0x1234, -1, 0x1234, -1, 0x1234, 0x1234, None, None, None) == C.MPI_ERR_ARG


def test_plan_path_0_and_1_contiguous_pieces(L, T):
    F = C.MPI_FLOAT
    assert _plan(L, 0, F, 5, F, 5, F, C.MPI_SUM) == (0, 0, 0, 0)
    for op in (C.MPI_SUM, C.MPI_REPLACE, C.MPI_NO_OP):
        assert _plan(L, 100, F, 100, F, 100, F, op) == (0, 100, 1, 4)
    assert _plan(L, 10, T["c10"], 200, F, 100, F, C.MPI_MAX) == (0, 100, 1, 4)
    assert _plan(L, 100, F, 10, T["c10"], 20, T["c10"], C.MPI_REPLACE) == (0, 100, 1, 4)
    # inside the first run of a strided result and target: one piece each
    assert _plan(L, 3, F, 1, T["v6x5"], 1, T["v6x5"], C.MPI_SUM) == (0, 3, 1, 4)
    assert _plan(L, 5, F, 1, T["v6x5"], 1, T["v6x5"], C.MPI_SUM) == (0, 5, 3, 4)       # one element past it
    for dt, esz, op in ((C.MPI_INT8_T, 1, C.MPI_SUM), (C.MSX_FLOAT16, 2, C.MPI_MAX), (C.MPI_DOUBLE, 8, C.MPI_PROD),
                        (C.MPI_C_DOUBLE_COMPLEX, 16, C.MPI_SUM), (C.MPI_2INT, 8, C.MPI_MAXLOC)):
        assert _plan(L, 10, dt, 10, dt, 10, dt, op) == (0, 10, 1, esz)
        assert _plan(L, 10, dt, 10, dt, 10, dt, C.MPI_REPLACE) == (0, 10, 1, esz)


def test_plan_path_3_the_three_layout_kernel(L, T):
    F = C.MPI_FLOAT
    # the vector of 16-byte blocks at a 32-byte stride
    assert _plan(L, 1, T["v16"], 1, T["v16"], 1, T["v16"], C.MPI_SUM) == (0, 148, 3, 4)
    assert _plan(L, 1, T["v16"], 1, T["v16"], 1, T["v16"], C.MPI_REPLACE) == (0, 148, 3, 16)
    # one side strided is enough, whichever it is
    assert _plan(L, 1, T["v16"], 148, F, 148, F, C.MPI_SUM) == (0, 148, 3, 4)
    assert _plan(L, 148, F, 1, T["v16"], 148, F, C.MPI_SUM) == (0, 148, 3, 4)
    assert _plan(L, 148, F, 148, F, 1, T["v16"], C.MPI_SUM) == (0, 148, 3, 4)
    # the 3-D subarray (60 elements in rows of 20 bytes; MPI_LB / MPI_UB are no elements)
    assert _plan(L, 2, T["sub"], 2, T["sub"], 2, T["sub"], C.MPI_SUM) == (0, 120, 3, 4)
    assert _plan(L, 2, T["sub"], 120, F, 1, T["v16"], C.MPI_REPLACE) == (0, 120, 3, 4)
    # an irregular indexed type, on one side and on all three
    assert _plan(L, 2, T["ix"], 1, T["v3"], 1, T["v5"], C.MPI_MIN) == (0, 28, 3, 4)
    assert _plan(L, 1, T["ix"], 1, T["ix"], 1, T["ix"], C.MPI_PROD) == (0, 14, 3, 4)
    # an origin smaller than the target and a result larger than n
    assert _plan(L, 1, T["v3"], 4, T["v16"], 2, T["v5"], C.MPI_SUM) == (0, 37, 3, 4)


def test_plan_granule_of_replace(L, T):
    # the largest power of two <= 16 common to the three layouts
    assert _plan(L, 1, T["b2"], 1, T["b2"], 1, T["b2"], C.MPI_REPLACE) == (0, 74, 3, 2)
    assert _plan(L, 1, T["b2"], 1, T["b2"], 74, T["b1"], C.MPI_REPLACE) == (0, 74, 3, 1)
    assert _plan(L, 8, T["v16"], 8, T["v16"], 64, T["b2"], C.MPI_REPLACE)[2:] == (3, 2)
    # a mixed struct (int8 at 0, double at 8: runs of 1 and 8 bytes) moves byte by byte
    assert _plan(L, 4, T["mixed"], 4, T["mixed"], 4, T["mixed"], C.MPI_REPLACE) == (0, 8, 3, 1)
    assert _plan(L, 16, T["mixed"], 1, T["v16"], 9, T["v16"], C.MPI_REPLACE) == (0, 32, 3, 1)


def test_plan_of_no_op_counts_the_result_triple(L, T):
    F = C.MPI_FLOAT
    # path 2: a typed -> typed copy target -> result; the origin triple may be anything
    for oc, odt in ((1, T["v16"]), (-9, 0x1234), (1 << 62, T["raw"]), (0, C.MPI_DATATYPE_NULL)):
        assert _plan(L, oc, odt, 2, T["v16"], 3, T["v16"], C.MPI_NO_OP) == (0, 296, 2, 16)
        assert _plan(L, oc, odt, 2, T["v3"], 3, T["v16"], C.MPI_NO_OP) == (0, 74, 2, 4)
        assert _plan(L, oc, odt, 74, F, 3, T["v16"], C.MPI_NO_OP) == (0, 74, 2, 4)
    # any committed types: a mixed struct copies byte by byte
    assert _plan(L, 0, 0, 4, T["mixed"], 1, T["v16"], C.MPI_NO_OP) == (0, 8, 2, 1)
    # an op takes n from the origin triple
    assert _plan(L, 1, T["v3"], 2, T["v16"], 3, T["v16"], C.MPI_SUM)[1] == 37


# ---- the plan entry never initialises a GPU ------------------------------------------

PLAN_WORKER = """
    import ctypes, os, sys
    sys.path.insert(0, os.path.join(REPO, "microsoft-mpi_amd"))
    import msx
    C = msx.C
    L = msx.init(errors_return=True)
    def gpu_fds():
        out = set()
        for fd in os.listdir("/proc/self/fd"):
            try:
                t = os.readlink("/proc/self/fd/" + fd)
            except OSError:
                continue
            if t.startswith("/dev/kfd") or t.startswith("/dev/dri"):
                out.add(t)
        return out
    before = gpu_fds()
    t = ctypes.c_int()
    assert L.MPI_Type_vector(37, 4, 8, C.MPI_FLOAT, ctypes.byref(t)) == 0
    assert L.MPI_Type_commit(ctypes.byref(t)) == 0
    n, path, gran = ctypes.c_int64(), ctypes.c_int(), ctypes.c_int()
    got = []
    for a in ((100, C.MPI_FLOAT, 100, C.MPI_FLOAT, 100, C.MPI_FLOAT, C.MPI_SUM),
              (1, t.value, 1, t.value, 1, t.value, C.MPI_SUM),
              (1, t.value, 1, t.value, 1, t.value, C.MPI_REPLACE),
              (0, 0, 1, t.value, 1, t.value, C.MPI_NO_OP),
              (2, t.value, 1, t.value, 1, t.value, C.MPI_SUM)):
        rc = L.msx_get_accumulate_plan(*a, ctypes.byref(n), ctypes.byref(path), ctypes.byref(gran))
        got.append((rc, n.value, path.value, gran.value))
    # the real calls up to their last host check
    assert L.msx_get_accumulate_dev(None, 1, t.value, None, 1, t.value, None, 1, t.value, C.MPI_SUM, None) == C.MPI_ERR_BUFFER
    assert L.msx_fetch_and_op_dev(None, None, None, 4, C.MPI_FLOAT, C.MPI_SUM, None) == C.MPI_ERR_BUFFER
    assert gpu_fds() == before, (before, gpu_fds())
    print("PLANS", got, "GPU_FDS", sorted(before))
"""


def test_plan_entry_and_host_checks_open_no_gpu():
    """In a fresh process that has not asked for the device count: after the
    plan entry and the calls' host checks the process holds no GPU device file
    it did not hold before them (on a host without a GPU there is none to open)."""
    pr = subprocess.run([sys.executable, "-c", f"REPO={msx.REPO_ROOT!r}\n" + textwrap.dedent(PLAN_WORKER)],
                        capture_output=True, text=True, timeout=120)
    assert pr.returncode == 0, pr.stdout + pr.stderr
    assert f"PLANS [(0, 100, 1, 4), (0, 148, 3, 4), (0, 148, 3, 16), (0, 148, 2, 16), ({C.MPI_ERR_TRUNCATE}, 0, 0, 0)]" \
        in pr.stdout, pr.stdout
