"""CPU, no GPU: the checks that the four plan entries of the typed accumulate
family share (include/msx.h: msx_accumulate_plan, msx_accumulate_widen_plan,
msx_accumulate_batch_plan, msx_get_accumulate_plan) give one class and one
message, whichever entry runs them.

Each case feeds the same broken argument to all four entries.  The messages are
compared after two adjustments: what an entry says about itself, its name with
the parenthesised reason that follows the name in the MSX_SUM_WIDE refusal,
becomes a placeholder, and the batch form's "segment N: " prefix is dropped.
One text is the batch form's own: it reports a negative count as "negative
count in segment N", so that case compares its class with the others' and its
text with the segment it names.  Truncation texts differ per entry by design
and are not compared.  The widening entry runs every shared check that comes
before its own element-type rule; all nine do."""
import ctypes
import re

import pytest

import msx
from test_accumulate_dev_cpu import L, T, device_op, user_op  # noqa: F401  (fixtures)

C = msx.C
i64, c_int = ctypes.c_int64, ctypes.c_int
F = C.MPI_FLOAT


def _arr(ct, vals):
    return (ct * len(vals))(*vals)


def _acc(L, oc, odt, tc, tdt, op):
    n, path, gran = i64(), c_int(), c_int()
    return L.msx_accumulate_plan(oc, odt, tc, tdt, op, ctypes.byref(n), ctypes.byref(path), ctypes.byref(gran))


def _widen(L, oc, odt, tc, tdt, op):
    n, path = i64(), c_int()
    return L.msx_accumulate_widen_plan(oc, odt, tc, tdt, op, ctypes.byref(n), ctypes.byref(path))


def _batch(L, oc, odt, tc, tdt, op):
    # the broken segment behind a good one: the text names segment 1
    out = [c_int(), i64(), c_int(), c_int(), c_int()]
    return L.msx_accumulate_batch_plan(_arr(i64, [1, oc]), _arr(c_int, [F, odt]), _arr(i64, [1, tc]),
                                       _arr(c_int, [F, tdt]), 2, op, *[ctypes.byref(o) for o in out])


def _gacc(L, oc, odt, tc, tdt, op):
    # the result triple is the target's
    n, path, gran = i64(), c_int(), c_int()
    return L.msx_get_accumulate_plan(oc, odt, tc, tdt, tc, tdt, op, ctypes.byref(n), ctypes.byref(path),
                                     ctypes.byref(gran))


ENTRIES = {"accumulate": _acc, "widen": _widen, "batch": _batch, "get_accumulate": _gacc}


def _normal(err):
    err = re.sub(r"^segment \d+: ", "", err)
    return re.sub(r"msx_\w+_dev( \([^)]*\))?", "<entry>", err)


def _all(L, *args):
    """{entry: (rc, normalised message)} for one set of arguments."""
    out = {}
    for name, fn in ENTRIES.items():
        rc = fn(L, *args)
        out[name] = (rc, _normal(msx.last_error()))
    return out


def _one_answer(L, want_rc, want_text, *args):
    got = _all(L, *args)
    assert {rc for rc, _ in got.values()} == {want_rc}, got
    assert len({err for _, err in got.values()}) == 1, got
    assert want_text in got["accumulate"][1], got
    return got["accumulate"][1]


def test_negative_count(L):
    got = _all(L, -1, F, 1, F, C.MPI_SUM)
    assert {rc for rc, _ in got.values()} == {C.MPI_ERR_COUNT}, got
    assert len({got[k][1] for k in ("accumulate", "widen", "get_accumulate")}) == 1, got
    assert got["accumulate"][1] == "negative count"
    assert got["batch"][1] == "negative count in segment 1"


def test_invalid_handle(L):
    _one_answer(L, C.MPI_ERR_TYPE, "invalid datatype 0x1234", 1, 0x1234, 1, F, C.MPI_SUM)
    _one_answer(L, C.MPI_ERR_TYPE, "null datatype", 1, F, 1, C.MPI_DATATYPE_NULL, C.MPI_SUM)


def test_uncommitted_type(L, T):
    for args in ((1, T["raw"], 1, F), (1, F, 1, T["raw"])):
        err = _one_answer(L, C.MPI_ERR_TYPE, "is not committed", *args, C.MPI_SUM)
        assert "0x%x" % (T["raw"] & 0xffffffff) in err


def test_user_op_and_device_op(L, user_op, device_op):
    for op in (user_op, device_op):
        assert _one_answer(L, C.MPI_ERR_OP, "builtin ops only", 1, F, 1, F, op) == "<entry> takes builtin ops only"


def test_sum_wide(L):
    err = _one_answer(L, C.MPI_ERR_OP, "MSX_SUM_WIDE", 1, C.MSX_FLOAT16, 2, F, C.MSX_SUM_WIDE)
    assert err == "MSX_SUM_WIDE is not defined for <entry>"


def test_op_null(L):
    _one_answer(L, C.MPI_ERR_OP, "MPI_Op", 1, F, 1, F, C.MPI_OP_NULL)


def test_count_overflow(L):
    # 2^61 floats are 2^63 bytes
    assert _one_answer(L, C.MPI_ERR_COUNT, "overflows", 1 << 61, F, 1 << 61, F, C.MPI_SUM) == \
        "count overflows the data size"
    assert _one_answer(L, C.MPI_ERR_COUNT, "overflows", 1, F, 1 << 61, F, C.MPI_SUM) == "count overflows the data size"


def test_mixed_struct_under_sum(L, T):
    # 9 data bytes into 18: no entry truncates, the widening one included
    err = _one_answer(L, C.MPI_ERR_TYPE, "no single basic element type", 1, T["mixed"], 2, T["mixed"], C.MPI_SUM)
    assert err == "origin datatype has no single basic element type"
