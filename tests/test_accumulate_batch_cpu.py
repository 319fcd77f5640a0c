"""CPU, no GPU: msx_accumulate_batch_dev / msx_accumulate_batch_plan
(include/msx.h): the two symbols, the order of the ten host-side checks, the
segment index in the error text, msx_accumulate_dev's classes with nseg == 1,
and the plan's figures.

Every check-order case breaks one check and at least one later one; the class
that comes back names the check that ran first.  The plan is a pure function
of its arguments and takes no addresses, so it runs without a GPU; the real
call is driven only into its checks (null or fake addresses are never
dereferenced there) and, without a GPU, to MPI_ERR_OTHER."""
import ctypes

import os
import re

import pytest

import msx
from test_accumulate_dev_cpu import BASE, FAR, L, T, device_op, user_op  # noqa: F401  (fixtures)

C = msx.C
vp, i64, c_int = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
F = C.MPI_FLOAT


def _arr(ct, vals):
    return (ct * max(len(vals), 1))(*vals)


def _args(segs):
    """segs: (origin, ocount, otype, target, tcount, ttype) per segment -> the six host arrays."""
    return (_arr(vp, [s[0] for s in segs]), _arr(i64, [s[1] for s in segs]), _arr(c_int, [s[2] for s in segs]),
            _arr(vp, [s[3] for s in segs]), _arr(i64, [s[4] for s in segs]), _arr(c_int, [s[5] for s in segs]))


def _plan(L, segs, op):
    """(rc, width, fuse_below, launches, batched, single); segs without addresses."""
    a = _args([(None, s[0], s[1], None, s[2], s[3]) for s in segs])
    w, fb, la, ba, si = c_int(-7), i64(-7), c_int(-7), c_int(-7), c_int(-7)
    rc = L.msx_accumulate_batch_plan(a[1], a[2], a[4], a[5], len(segs), op, ctypes.byref(w), ctypes.byref(fb),
                                     ctypes.byref(la), ctypes.byref(ba), ctypes.byref(si))
    return rc, w.value, fb.value, la.value, ba.value, si.value


def _call(L, segs, op):
    a = _args(segs)
    rc = L.msx_accumulate_batch_dev(*a, len(segs), op, None)
    return rc, msx.last_error()


def _both(L, segs, op):
    """The class both entry points return for segments that fail one of checks 2 - 7."""
    rc, err = _call(L, segs, op)
    assert rc != 0
    assert _plan(L, [(s[1], s[2], s[4], s[5]) for s in segs], op)[0] == rc
    return rc, err


def _seg(oc, odt, tc, tdt, k=0, origin=True, target=True):
    """One segment with fake, distinct, 16-byte aligned addresses."""
    return (FAR + (k << 24) if origin else None, oc, odt, BASE + (k << 24) if target else None, tc, tdt)


@pytest.fixture(scope="module")
def limits(L):
    rc, width, fuse_below, *_ = _plan(L, [], C.MPI_SUM)
    assert rc == 0
    return width, fuse_below


# ---- the symbols -------------------------------------------------------------------

def test_both_symbols_are_exported_and_declared(L):
    with open(os.path.join(msx.INCLUDE_DIR, "msx.h")) as f:
        txt = f.read()
    for name in ("msx_accumulate_batch_dev", "msx_accumulate_batch_plan"):
        assert hasattr(L, name)
        assert name in msx.exported_symbols()
        assert re.search(r"^int %s\(" % name, txt, re.M)


# ---- the order of the checks -------------------------------------------------------

def test_no_segments_succeed_before_everything(L):
    # check 1, with null arrays, a bad op and no GPU behind it
    assert L.msx_accumulate_batch_dev(None, None, None, None, None, None, 0, 0x1234, None) == 0
    assert _plan(L, [], 0x1234)[0] == 0


def test_the_arrays_come_before_the_counts(L, T):
    # check 2, with a negative count, a bad datatype and a bad op behind it
    a = _args([_seg(-1, 0x1234, -1, T["raw"])])
    out = [c_int(), i64(), c_int(), c_int(), c_int()]
    refs = [ctypes.byref(o) for o in out]
    for hole in range(6):
        b = list(a)
        b[hole] = None
        assert L.msx_accumulate_batch_dev(*b, 1, 0x1234, None) == C.MPI_ERR_ARG
        if hole not in (0, 3):
            assert L.msx_accumulate_batch_plan(b[1], b[2], b[4], b[5], 1, 0x1234, *refs) == C.MPI_ERR_ARG
    assert L.msx_accumulate_batch_dev(*a, -1, 0x1234, None) == C.MPI_ERR_ARG
    assert L.msx_accumulate_batch_plan(a[1], a[2], a[4], a[5], -1, 0x1234, *refs) == C.MPI_ERR_ARG


def test_counts_come_before_the_datatypes(L, T):
    # check 3 in a later segment than a bad datatype (check 4), a bad op and truncation behind it
    segs = [_seg(9, 0x1234, 1, T["vi3"], 0), _seg(1, T["raw"], 1, T["v3"], 1), _seg(1, T["v5"], -1, T["v3"], 2)]
    rc, err = _both(L, segs, 0x1234)
    assert rc == C.MPI_ERR_COUNT and "segment 2" in err
    rc, err = _both(L, [_seg(1, T["v5"], 1, T["v3"], 0), _seg(-4, T["v5"], 1, T["v3"], 1)], C.MPI_SUM)
    assert rc == C.MPI_ERR_COUNT and "segment 1" in err


def test_datatypes_come_before_the_op(L, T, user_op):
    # check 4, with a bad op, truncation, unlike element kinds and null buffers behind it
    good = _seg(1, T["v5"], 1, T["v3"], 0)
    for op in (0x1234, user_op, C.MSX_SUM_WIDE, C.MPI_SUM):
        rc, err = _both(L, [good, _seg(9, 0x1234, 1, T["vi3"], 1, origin=False)], op)
        assert rc == C.MPI_ERR_TYPE and "segment 1" in err
        rc, err = _both(L, [good, good, _seg(9, T["v5"], 1, C.MPI_DATATYPE_NULL, 2)], op)
        assert rc == C.MPI_ERR_TYPE and "segment 2" in err
        rc, err = _both(L, [_seg(9, T["raw"], 1, T["vi3"], 0), good], op)
        assert rc == C.MPI_ERR_TYPE and "not committed" in err and "segment 0" in err
        rc, err = _both(L, [good, _seg(9, T["v5"], 1, T["raw"], 1)], op)
        assert rc == C.MPI_ERR_TYPE and "not committed" in err and "segment 1" in err


def test_the_op_comes_before_truncation_and_the_element_types(L, T, user_op, device_op):
    # check 5: 9 x 37 floats into 1 x 37 ints behind it (truncation, unlike kinds, null buffers)
    segs = [_seg(1, T["v5"], 1, T["v3"], 0), _seg(9, T["v5"], 1, T["vi3"], 1, target=False)]
    assert _both(L, segs, 0x1234)[0] == C.MPI_ERR_OP
    assert _both(L, segs, C.MPI_OP_NULL)[0] == C.MPI_ERR_OP
    for op in (user_op, device_op):
        rc, err = _both(L, segs, op)
        assert rc == C.MPI_ERR_OP and "builtin ops only" in err
    rc, err = _both(L, segs, C.MSX_SUM_WIDE)
    assert rc == C.MPI_ERR_OP and "MSX_SUM_WIDE" in err
    rc, err = _both(L, [_seg(4, C.MSX_BFLOAT16, 4, C.MSX_BFLOAT16)], C.MSX_SUM_WIDE)
    assert rc == C.MPI_ERR_OP and "MSX_SUM_WIDE" in err


def test_the_per_segment_checks_run_in_index_order(L, T):
    # check 6: the first failing segment decides, whatever fails in a later one;
    # unlike kinds between segments (check 7) and null buffers behind it
    trunc = lambda k: _seg(2, T["v5"], 1, T["v3"], k, origin=False)
    kind = lambda k: _seg(1, T["v5"], 1, T["vi3"], k)
    pair = lambda k: _seg(1, T["b1"], 1, T["b1"], k)              # MPI_SUM on MPI_BYTE
    ints = lambda k: _seg(1, T["vi3"], 1, T["vi3"], k)
    good = lambda k: _seg(1, T["v5"], 1, T["v3"], k)
    rc, err = _both(L, [good(0), ints(1), trunc(2), kind(3)], C.MPI_SUM)
    assert rc == C.MPI_ERR_TRUNCATE and "segment 2" in err and "296" in err and "148" in err
    rc, err = _both(L, [good(0), kind(1), trunc(2)], C.MPI_SUM)
    assert rc == C.MPI_ERR_TYPE and "segment 1" in err and "kind" in err
    rc, err = _both(L, [good(0), ints(1), pair(2), trunc(3)], C.MPI_SUM)
    assert rc == C.MPI_ERR_OP and "segment 2" in err
    rc, err = _both(L, [good(0), _seg(1, T["vfi"], 1, T["vfi"], 1)], C.MPI_MAXLOC)
    assert rc == C.MPI_ERR_OP and "segment 0" in err                       # MAXLOC on floats comes first
    rc, err = _both(L, [_seg(1, T["mixed"], 1, T["mixed"], 0), trunc(1)], C.MPI_SUM)
    assert rc == C.MPI_ERR_TYPE and "segment 0" in err and "no single basic element type" in err
    # data bytes beyond 2^62
    rc, err = _both(L, [good(0), _seg(1 << 61, C.MPI_DOUBLE, 1 << 61, C.MPI_DOUBLE, 1)], C.MPI_SUM)
    assert rc == C.MPI_ERR_COUNT and "segment 1" in err
    # MPI_NO_OP is looked at after the sizes, and an empty segment before its element types
    rc, err = _both(L, [good(0), trunc(1)], C.MPI_NO_OP)
    assert rc == C.MPI_ERR_TRUNCATE and "segment 1" in err
    empty = [(None, 0, T["vfi"], None, 3, T["mixed"]), (None, 0, T["v5"], None, 0, T["vi3"])]
    assert _call(L, empty, C.MPI_MAXLOC)[0] == 0
    assert _plan(L, [(s[1], s[2], s[4], s[5]) for s in empty], C.MPI_MAXLOC)[3:] == (0, 0, 0)
    # under MPI_NO_OP the call succeeds here: mixed kinds, null buffers and no GPU are behind it
    noop = [(None, 1, T["v5"], None, 1, T["vi3"]), (None, 1, T["mixed"], None, 2, T["v5"]), (None, 3, F, None, 3, F)]
    assert _call(L, noop, C.MPI_NO_OP)[0] == 0


def test_one_element_kind_comes_before_the_buffers(L, T):
    # check 7 with null buffers and identical targets behind it; the error names both segments
    segs = [(None, 0, T["vi3"], None, 0, T["vi3"]),                         # empty: no kind
            _seg(1, T["v5"], 1, T["v3"], 1, origin=False), _seg(3, F, 3, F, 2),
            _seg(1, T["vi3"], 1, T["vi3"], 1), _seg(2, C.MPI_DOUBLE, 2, C.MPI_DOUBLE, 4)]
    rc, err = _both(L, segs, C.MPI_SUM)
    assert rc == C.MPI_ERR_TYPE and "segment 1" in err and "segment 3" in err
    # MPI_REPLACE asks nothing of the element types: the same segments reach the buffer check
    rc, err = _call(L, segs, C.MPI_REPLACE)
    assert rc == C.MPI_ERR_BUFFER and "null" in err and "segment 1" in err
    assert _plan(L, [(s[1], s[2], s[4], s[5]) for s in segs], C.MPI_REPLACE)[0] == 0
    # the same element kind under two datatype names is one kind
    assert _plan(L, [(3, C.MPI_INT, 3, C.MPI_INT), (1, T["vi3"], 37, C.MPI_INT32_T)], C.MPI_SUM)[0] == 0


def test_null_buffers_come_before_identical_targets(L, T):
    # check 8 with check 9 (and, without a GPU, check 10) behind it
    same = _seg(1, T["v5"], 1, T["v3"], 0)
    for origin, target in ((False, True), (True, False), (False, False)):
        segs = [same, same, (None, 0, T["v5"], None, 1, T["v3"]), _seg(1, T["v5"], 1, T["v3"], 3, origin, target)]
        assert _plan(L, [(s[1], s[2], s[4], s[5]) for s in segs], C.MPI_SUM)[0] == 0
        rc, err = _call(L, segs, C.MPI_SUM)
        assert rc == C.MPI_ERR_BUFFER and "null" in err and "segment 3" in err


def test_identical_targets_come_before_the_gpu(L, T):
    # check 9: same target address and same target datatype handle
    a = _seg(1, T["v5"], 1, T["v3"], 0)
    b = (FAR + 64, 37, F, a[3], 1, T["v3"])
    rc, err = _call(L, [_seg(3, F, 3, F, 5), a, _seg(1, T["v5"], 1, T["v3"], 2), b], C.MPI_SUM)
    assert rc == C.MPI_ERR_BUFFER and "segment 1" in err and "segment 3" in err
    # an empty segment collides with nothing
    rc, err = _call(L, [a, (None, 0, F, a[3], 1, T["v3"]), a], C.MPI_REPLACE)
    assert rc == C.MPI_ERR_BUFFER and "segment 0" in err and "segment 2" in err


def test_valid_arguments_without_a_gpu_are_mpi_err_other(L, T):
    if L.msx_device_count() > 0:
        pytest.skip("GPU present")
    # one address with two datatype handles, and one handle at two addresses, pass check 9
    segs = [_seg(1, T["v5"], 1, T["v3"], 0), (FAR, 37, F, BASE, 1, T["v2x60"]), _seg(1, T["ix"], 1, T["v3"], 2),
            (None, 0, F, None, 0, F), _seg(100, F, 100, F, 4)]
    assert _plan(L, [(s[1], s[2], s[4], s[5]) for s in segs], C.MPI_SUM)[3:] == (1, 4, 0)
    assert _call(L, segs, C.MPI_SUM)[0] == C.MPI_ERR_OTHER
    assert _call(L, segs, C.MPI_REPLACE)[0] == C.MPI_ERR_OTHER


# ---- nseg == 1: msx_accumulate_dev's classes -----------------------------------------

def _single_cases(T, user_op, device_op):
    """Every failing argument set of test_accumulate_dev_cpu.py's check-order cases:
    (origin_count, origin_type, target_count, target_type, op)."""
    out = []
    for oc, tc in ((-1, 1), (1, -1), (-5, -5)):
        out += [(oc, 0x1234, tc, T["raw"], 0x1234), (oc, T["v5"], tc, T["v3"], C.MPI_SUM)]
    for op in (0x1234, user_op, C.MSX_SUM_WIDE, C.MPI_SUM):
        out += [(9, 0x1234, 1, T["vi3"], op), (9, T["v5"], 1, C.MPI_DATATYPE_NULL, op),
                (9, T["raw"], 1, T["vi3"], op), (9, T["v5"], 1, T["raw"], op)]
    for op in (0x1234, C.MPI_OP_NULL, user_op, device_op, C.MSX_SUM_WIDE):
        out.append((9, T["v5"], 1, T["vi3"], op))
    out.append((4, C.MSX_BFLOAT16, 4, C.MSX_BFLOAT16, C.MSX_SUM_WIDE))
    for op in (C.MPI_SUM, C.MPI_BAND, C.MPI_REPLACE, C.MPI_NO_OP):
        out.append((2, T["v5"], 1, T["vi3"], op))
    out += [(1, T["v5"], 0, T["vi3"], C.MPI_SUM), (1, C.MPI_DOUBLE, 1, F, C.MPI_SUM),
            (1, T["v5"], 1, T["vi3"], C.MPI_SUM), (1, T["v5"], 1, T["vi3"], C.MPI_BAND),
            (1, T["vfi"], 1, T["vfi"], C.MPI_MAXLOC), (1, T["mixed"], 1, T["mixed"], C.MPI_SUM),
            (4, F, 1, T["vfi"], C.MPI_SUM), (1, T["v5"], 1, T["v3"], C.MPI_BAND), (1, T["v5"], 1, T["v3"], C.MPI_MAXLOC),
            (1, T["b1"], 1, T["b1"], C.MPI_SUM), (4, C.MSX_FLOAT16, 4, C.MSX_FLOAT16, C.MPI_LAND)]
    return out


def test_one_segment_returns_the_single_calls_class(L, T, user_op, device_op):
    for oc, odt, tc, tdt, op in _single_cases(T, user_op, device_op):
        for origin, target in ((None, None), (FAR, BASE)):
            want = L.msx_accumulate_dev(origin, oc, odt, target, tc, tdt, op, None)
            assert want != 0
            rc, err = _call(L, [(origin, oc, odt, target, tc, tdt)], op)
            assert rc == want, (oc, odt, tc, tdt, op, err)
    # null buffers behind passing checks, and what succeeds without looking at them
    for a in ((1, T["v5"], 1, T["v3"], C.MPI_SUM), (100, F, 100, F, C.MPI_SUM), (1, T["b2"], 1, T["b16"], C.MPI_REPLACE),
              (1, T["v5"], 3, T["vi3"], C.MPI_REPLACE), (0, T["v5"], 3, T["vi3"], C.MPI_SUM),
              (1, T["mixed"], 2, T["v5"], C.MPI_NO_OP)):
        for origin, target in ((None, BASE), (FAR, None), (None, None)):
            want = L.msx_accumulate_dev(origin, a[0], a[1], target, a[2], a[3], a[4], None)
            assert want in (0, C.MPI_ERR_BUFFER)
            assert _call(L, [(origin, a[0], a[1], target, a[2], a[3])], a[4])[0] == want
    if L.msx_device_count() == 0:
        a = (1, T["v5"], 1, T["v3"])
        assert L.msx_accumulate_dev(FAR, a[0], a[1], BASE, a[2], a[3], C.MPI_SUM, None) == C.MPI_ERR_OTHER
        assert _call(L, [(FAR, a[0], a[1], BASE, a[2], a[3])], C.MPI_SUM)[0] == C.MPI_ERR_OTHER


# ---- the plan's figures ------------------------------------------------------------

def test_plan_outputs_are_required(L, T):
    a = _args([_seg(1, T["v5"], 1, T["v3"])])
    out = [c_int(), i64(), c_int(), c_int(), c_int()]
    for hole in range(5):
        refs = [ctypes.byref(o) for o in out]
        refs[hole] = None
        assert L.msx_accumulate_batch_plan(a[1], a[2], a[4], a[5], 1, C.MPI_SUM, *refs) == C.MPI_ERR_ARG
    # before every other check, also with no segments
    assert L.msx_accumulate_batch_plan(None, None, None, None, 0, 0x1234, None, None, None, None, None) == C.MPI_ERR_ARG


def test_width_and_fuse_below(limits):
    width, fuse_below = limits
    assert width >= 8                      # a block's six faces fit one launch
    assert fuse_below > 0


def test_launches_at_the_width_edges(L, T, limits):
    width, _ = limits
    for n in (1, width, width + 1, 2 * width + 3):
        rc, w, _, launches, batched, single = _plan(L, [(1, T["v5"], 1, T["v3"])] * n, C.MPI_SUM)
        assert (rc, w, batched, single) == (0, width, n, 0)
        assert launches == -(-batched // width) + single == -(-n // width)


def test_every_path_of_the_single_call_is_fused(L, T):
    # msx_accumulate_plan's paths 1, 2, 4 under an op and 1, 2, 3, 4 under MPI_REPLACE, predefined handles included
    segs = [(100, F, 100, F), (10, T["c10"], 200, F), (111, F, 3, T["v3"]), (1, T["v5"], 37, F), (1, T["ix"], 1, T["v3"]),
            (2, T["sub"], 4, T["v3"])]
    for op in (C.MPI_SUM, C.MPI_REPLACE):
        assert _plan(L, segs, op)[3:] == (1, len(segs), 0)


def test_empty_segments_are_counted_nowhere(L, T, limits):
    width, _ = limits
    e1, e2, e3 = (0, T["v5"], 3, T["v3"]), (0, T["vfi"], 0, T["mixed"]), (5, T["v5"], 0, 0)
    assert _plan(L, [e3], C.MPI_SUM)[0] == C.MPI_ERR_TYPE          # a bad handle is still looked at
    segs = [e1] + [(1, T["v5"], 1, T["v3"])] * width + [e2, (3, F, 3, F), e1]
    assert _plan(L, segs, C.MPI_SUM)[3:] == (2, width + 1, 0)
    assert _plan(L, [e1, e2, e1], C.MPI_SUM)[3:] == (0, 0, 0)


def test_the_fuse_limit_is_exclusive(L, T, limits):
    width, fuse_below = limits
    assert fuse_below % 8 == 0
    at, under = fuse_below // 4, fuse_below // 4 - 1
    small = (1, T["v5"], 1, T["v3"])
    assert _plan(L, [small, (at, F, at, F), small], C.MPI_SUM)[3:] == (2, 2, 1)
    assert _plan(L, [small, (under, F, under, F), small], C.MPI_SUM)[3:] == (1, 3, 0)
    assert _plan(L, [(at, F, at, F)] * 3 + [small] * (width + 1), C.MPI_SUM)[3:] == (5, width + 1, 3)
    # data bytes of the origin decide, not the target's size
    assert _plan(L, [(under, F, 4 * at, F)], C.MPI_SUM)[3:] == (1, 1, 0)
    assert _plan(L, [(fuse_below, C.MPI_BYTE, fuse_below, C.MPI_BYTE)], C.MPI_REPLACE)[3:] == (1, 0, 1)
    assert _plan(L, [(fuse_below - 1, C.MPI_BYTE, fuse_below, C.MPI_BYTE)], C.MPI_REPLACE)[3:] == (1, 1, 0)


def test_no_op_gives_no_launches(L, T):
    segs = [(1, T["v5"], 1, T["vi3"]), (3, T["mixed"], 1, T["v5"]), (100, F, 100, F)]
    assert _plan(L, segs, C.MPI_NO_OP)[3:] == (0, 0, 0)


def test_mixed_element_kinds(L, T):
    segs = [(1, T["v5"], 1, T["v3"]), (1, T["vi3"], 1, T["vi3"]), (2, T["mixed"], 1, T["b16"])]
    assert _plan(L, segs[:2], C.MPI_SUM)[0] == C.MPI_ERR_TYPE
    assert "segment 0" in msx.last_error() and "segment 1" in msx.last_error()
    assert _plan(L, segs, C.MPI_REPLACE)[3:] == (1, 3, 0)
    assert _plan(L, segs[:2], C.MPI_NO_OP)[3:] == (0, 0, 0)
