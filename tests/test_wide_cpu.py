"""CPU: MSX_SUM_WIDE (include/msx.h), the fp32-accumulated tree sum of
MSX_FLOAT16 / MSX_BFLOAT16: the handle, the legality table, the op's
attributes, the calls that refuse it, the header, and a self-test of the numpy
definition the GPU tests hold the kernels to (tests/_wide_ref.py).  No call
here needs a GPU."""
import ctypes
import json
import os
import subprocess

import numpy as np

import msx
import _half_ref as R
import _wide_ref as WR

C = msx.C
WIDE = C.MSX_SUM_WIDE          # every test below needs the constant
c_int = ctypes.c_int
u32 = lambda v: v & 0xFFFFFFFF
HALF = ("MSX_FLOAT16", "MSX_BFLOAT16")
ONE = {"MSX_FLOAT16": 0x3C00, "MSX_BFLOAT16": 0x3F80}
EPS = {"MSX_FLOAT16": 0x0C00, "MSX_BFLOAT16": 0x3B00}      # 2^-12, 2^-9: a quarter of an ulp of 1
MAXF = {"MSX_FLOAT16": 0x7BFF, "MSX_BFLOAT16": 0x7F7F}
INF = {"MSX_FLOAT16": 0x7C00, "MSX_BFLOAT16": 0x7F80}


def _u16(*v):
    return np.array(v, np.uint16)


def test_handle_value_layout_and_no_collision_with_mpi_h():
    assert u32(WIDE) == 0x58000050
    # builtin handle of kind MPID_OP, like MPI_SUM, nothing in the middle bytes
    assert u32(WIDE) & ~0xFF == u32(C.MPI_SUM) & ~0xFF and u32(WIDE) >> 30 == 1 and (u32(WIDE) >> 26) & 0xF == 6
    with open(os.path.join(msx.REPO_ROOT, "tests", "golden", "mpi_h_constants.json")) as f:
        golden = json.load(f)["constants"]
    taken = {u32(v) for v in golden.values()}
    taken |= {u32(v) for k, v in vars(C).items() if k.startswith("MPI_") and isinstance(v, int)}
    assert u32(WIDE) not in taken
    ops = [u32(v) & 0xFF for k, v in vars(C).items()
           if k.startswith("MPI_") and isinstance(v, int) and u32(v) & ~0xFF == u32(C.MPI_SUM) & ~0xFF]
    assert ops and max(ops) == 0x0E and 0x50 not in ops
    with open(os.path.join(msx.INCLUDE_DIR, "mpi.h")) as f:
        assert "MSX_SUM_WIDE" not in f.read()
    with open(os.path.join(msx.INCLUDE_DIR, "mpif.h")) as f:
        assert "MSX_SUM_WIDE" not in f.read()
    # the neighbouring indices stay invalid: 0x0f (the internal index) and 0x51
    L = msx.lib()
    for bad in (0x5800000F, 0x58000051, 0x58000150):
        assert L.msx_op_check(bad, C.MSX_BFLOAT16) == C.MPI_ERR_OP


def test_op_check_exactly_two_legal_pairs():
    L = msx.lib()
    with open(os.path.join(msx.REPO_ROOT, "tests", "golden", "mpi_h_constants.json")) as f:
        golden = json.load(f)["constants"]
    names = {k for k in golden if u32(golden[k]) >> 16 == 0x4C00}
    names |= {k for k, v in vars(C).items() if isinstance(v, int) and u32(v) >> 16 == 0x4C00}
    assert len(names) > 40 and set(HALF) <= names
    legal = sorted(n for n in names if L.msx_op_check(WIDE, getattr(C, n)) == C.MPI_SUCCESS)
    assert legal == sorted(HALF)
    for n in names - set(HALF):
        assert L.msx_op_check(WIDE, getattr(C, n)) == C.MPI_ERR_OP, n
    assert L.msx_op_check(WIDE, C.MPI_DATATYPE_NULL) != C.MPI_SUCCESS
    # MPI_SUM keeps its pairs
    assert L.msx_op_check(C.MPI_SUM, C.MPI_FLOAT) == C.MPI_SUCCESS
    assert L.msx_op_check(C.MPI_SUM, C.MSX_BFLOAT16) == C.MPI_SUCCESS


def test_commutative_not_freeable_and_not_in_the_op_table(msxlib):
    L = msxlib
    c = c_int(-1)
    assert L.MPI_Op_commutative(WIDE, ctypes.byref(c)) == 0 and c.value == 1
    h = c_int(WIDE)
    assert L.MPI_Op_free(ctypes.byref(h)) == C.MPI_ERR_OP and h.value == WIDE
    L.msx_op_table.restype = ctypes.c_void_p
    L.msx_op_table.argtypes = [c_int]
    assert L.msx_op_table(WIDE) is None
    assert L.msx_op_table(C.MPI_SUM) is not None
    assert L.msx_op_is_device(WIDE) == 0 and L.msx_op_has_device_tree(WIDE) == 0


def test_scans_and_one_sided_calls_refuse_the_op_by_name(msxlib):
    L = msxlib
    a = np.full(8, 0x3F80, np.uint16)
    b = np.full(8, 0x4000, np.uint16)
    D = C.MSX_BFLOAT16
    W = C.MPI_COMM_WORLD
    L.MPI_Scan.argtypes = [ctypes.c_void_p, ctypes.c_void_p, c_int, c_int, c_int, c_int]
    L.MPI_Exscan.argtypes = L.MPI_Scan.argtypes
    for fn in (L.MPI_Scan, L.MPI_Exscan):
        assert fn(a.ctypes.data, b.ctypes.data, 8, D, WIDE, W) == C.MPI_ERR_OP
        assert "MSX_SUM_WIDE" in msx.last_error()
        assert fn(a.ctypes.data, b.ctypes.data, 8, D, C.MPI_SUM, W) == 0      # one rank: a copy, no GPU needed
    for name in ("MPI_Iscan", "MPI_Iexscan"):
        fn = getattr(L, name)
        fn.argtypes = L.MPI_Scan.argtypes + [ctypes.c_void_p]
        req = c_int(-1)
        assert fn(a.ctypes.data, b.ctypes.data, 8, D, WIDE, W, ctypes.byref(req)) == C.MPI_ERR_OP
        assert "MSX_SUM_WIDE" in msx.last_error() and req.value == C.MPI_REQUEST_NULL
    assert (b == 0x3F80).all()            # the two MPI_SUM copies; no refused call wrote
    buf = np.zeros(64, np.uint16)
    res = np.zeros(8, np.uint16)
    win = c_int()
    assert L.MPI_Win_create(buf.ctypes.data, 128, 2, C.MPI_INFO_NULL, W, ctypes.byref(win)) == 0
    assert L.MPI_Win_set_errhandler(win, C.MPI_ERRORS_RETURN) == 0
    assert L.MPI_Accumulate(a.ctypes.data, 8, D, 0, 0, 8, D, WIDE, win) == C.MPI_ERR_OP
    assert "MSX_SUM_WIDE" in msx.last_error()
    assert L.MPI_Get_accumulate(a.ctypes.data, 8, D, res.ctypes.data, 8, D, 0, 0, 8, D, WIDE, win) == C.MPI_ERR_OP
    assert "MSX_SUM_WIDE" in msx.last_error()
    assert L.MPI_Fetch_and_op(a.ctypes.data, res.ctypes.data, D, 0, 0, WIDE, win) == C.MPI_ERR_OP
    assert "MSX_SUM_WIDE" in msx.last_error()
    assert L.MPI_Win_free(ctypes.byref(win)) == 0
    assert not buf.any() and not res.any()


def test_reduce_local_without_gpu_fails_loudly_and_float_is_err_op(msxlib):
    L = msxlib
    f = np.arange(8, dtype=np.float32)
    g = np.ones(8, np.float32)
    assert L.MPI_Reduce_local(f.ctypes.data, g.ctypes.data, 8, C.MPI_FLOAT, WIDE) == C.MPI_ERR_OP
    assert "MSX_SUM_WIDE" in msx.last_error() and (g == 1).all()
    assert L.msx_reduce_local_dev(f.ctypes.data, g.ctypes.data, 8, C.MPI_FLOAT, WIDE, None) == C.MPI_ERR_OP
    assert L.msx_reduce_local_multi(f.ctypes.data, g.ctypes.data, 8, C.MPI_FLOAT, WIDE, 1) == C.MPI_ERR_OP
    srcs = (ctypes.c_void_p * 2)(f.ctypes.data, g.ctypes.data)
    assert L.msx_reduce_tree_dev(srcs, 2, g.ctypes.data, 8, C.MPI_FLOAT, WIDE, None) == C.MPI_ERR_OP
    assert (g == 1).all()
    if L.msx_device_count() == 0:
        a = np.full(8, 0x3C00, np.uint16)
        b = np.full(8, 0x4000, np.uint16)
        for dt in HALF:
            rc = L.MPI_Reduce_local(a.ctypes.data, b.ctypes.data, 8, getattr(C, dt), WIDE)
            assert rc == C.MPI_ERR_OTHER and "no usable MI355X" in msx.last_error()
            srcs = (ctypes.c_void_p * 2)(a.ctypes.data, b.ctypes.data)
            assert L.msx_reduce_tree_dev(srcs, 2, b.ctypes.data, 8, getattr(C, dt), WIDE, None) == C.MPI_ERR_OTHER
        assert (b == 0x4000).all()


def test_plain_c_file_naming_the_constant_compiles(tmp_path):
    src = tmp_path / "wide.c"
    src.write_text("""
        #include "msx.h"
        static const MPI_Op ops[2] = {MPI_SUM, MSX_SUM_WIDE};
        int wide_legal(void)
        {
            switch (ops[1]) { case MSX_SUM_WIDE: break; case MPI_SUM: return -1; default: return -2; }
            return msx_op_check(ops[1], MSX_BFLOAT16) + msx_op_check(ops[0], MSX_FLOAT16);
        }
    """)
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", msx.INCLUDE_DIR, "-c",
                    str(src), "-o", str(tmp_path / "wide.o")], check=True)


# ---- the numpy definition on known answers ----------------------------------------
def _slots(srcs):
    s = [None] * (2 * len(srcs))
    s[0::2] = srcs
    return s


def test_reference_keeps_contributions_below_half_an_ulp():
    """1 + 7 * (ulp / 4): the per-node chain drops every small term (1), the
    per-node tree loses 1 + ulp/2 to a tie (1 + ulp); fp32 accumulation holds
    1 + 7/4 ulp and rounds once, to 1 + 2 ulp."""
    for dt in HALF:
        srcs = [_u16(ONE[dt])] + [_u16(EPS[dt])] * 7
        assert WR.tree(dt, srcs, 8, 0, 0, 1).tolist() == [ONE[dt] + 2]
        assert WR.tree(dt, _slots(srcs), 8, 0, 8, 0).tolist() == [ONE[dt] + 2]
        assert WR.balanced(dt, srcs).tolist() == [ONE[dt] + 2]
        assert R.tree("MPI_SUM", dt, srcs, 8, 0, 0, 1).tolist() == [ONE[dt]]
        assert R.tree("MPI_SUM", dt, _slots(srcs), 8, 0, 8, 0).tolist() == [ONE[dt] + 1]
    assert WR.tree("MSX_BFLOAT16", [_u16(0x3F80)] + [_u16(0x3B00)] * 7, 8, 0, 0, 1).tolist() == [0x3F82]
    assert R.tree("MPI_SUM", "MSX_BFLOAT16", [_u16(0x3F80)] + [_u16(0x3B00)] * 7, 8, 0, 0, 1).tolist() == [0x3F80]


def test_reference_two_sources_equal_mpi_sum_for_partner_pairs():
    for dt in HALF:
        p = R.partners(dt)
        a, b = np.repeat(p, p.size), np.tile(p, p.size)
        for io, x in ((a, b), (b, a)):
            exp = R.combine("MPI_SUM", dt, io, x)
            assert np.array_equal(WR.tree(dt, [io, x], 2, 0, 0, 1), exp)                    # chain
            assert np.array_equal(WR.tree(dt, [io, None, x, None], 2, 0, 2, 0), exp)        # two leaves
            assert np.array_equal(WR.tree(dt, [io, x], 1, 1, 1, 0), exp)                    # one leaf pair


def test_reference_one_source_returns_every_pattern_unchanged():
    every = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)
    for dt in HALF:
        assert np.array_equal(WR.tree(dt, [every, None], 1, 0, 1, 0), every)
        assert np.array_equal(WR.tree(dt, [every, None, None, None], 2, 0, 1, 0), every)    # absent right leaf
        assert np.array_equal(WR.tree(dt, [every], 1, 0, 0, 1), every)
        # widening is W wherever W is defined, and a NaN keeps sign and payload
        ok = (every & 0x7FFF) <= INF[dt]
        assert np.array_equal(WR.widen(dt, every)[ok], R.W[dt](every[ok]).view(np.uint32))
        assert np.isnan(WR.widen(dt, every)[~ok].view(np.float32)).all()


def test_reference_root_ties_to_even_and_rounds_once():
    for dt in HALF:
        one, q = ONE[dt], EPS[dt]                                                 # q = ulp / 4
        # 1 + 2 * ulp/4 is halfway between 1 (even) and 1 + ulp: down
        assert WR.tree(dt, [_u16(one), _u16(q), _u16(q)], 3, 0, 0, 1).tolist() == [one]
        # (1 + ulp) + 2 * ulp/4 is halfway between odd and even: up, where the
        # per-node rounding keeps 1 + ulp twice
        assert WR.tree(dt, [_u16(one + 1), _u16(q), _u16(q)], 3, 0, 0, 1).tolist() == [one + 2]
        assert R.tree("MPI_SUM", dt, [_u16(one + 1), _u16(q), _u16(q)], 3, 0, 0, 1).tolist() == [one + 1]


def test_reference_overflow_only_at_the_root_and_nan_rule():
    for dt in HALF:
        mx, inf, q = MAXF[dt], INF[dt], R.QBIT[dt]
        assert WR.tree(dt, [_u16(mx), _u16(mx)], 2, 0, 0, 1).tolist() == [inf]
        # fp16: fp32 holds 2 * max, adding -max comes back into range.  bf16 has
        # fp32's own exponent range, so 2 * max is inf in the fp32 partial too;
        # for bf16 the fp32 partial adds mantissa bits, not range
        back = mx if dt == "MSX_FLOAT16" else inf
        assert WR.tree(dt, [_u16(mx), _u16(mx), _u16(0x8000 | mx)], 3, 0, 0, 1).tolist() == [back]
        # max + ulp(max)/4 + ulp(max)/4 ties to the even neighbour, inf, only
        # because fp32 kept both quarters (2^(e - mant - 2): exponent field lowered)
        mant = 10 if dt == "MSX_FLOAT16" else 7
        qm = (mx & inf) - ((mant + 2) << mant)
        assert WR.tree(dt, [_u16(mx), _u16(qm), _u16(qm)], 3, 0, 0, 1).tolist() == [inf]
        assert R.tree("MPI_SUM", dt, [_u16(mx), _u16(qm), _u16(qm)], 3, 0, 0, 1).tolist() == [mx]
        assert R.tree("MPI_SUM", dt, [_u16(mx), _u16(mx), _u16(0x8000 | mx)], 3, 0, 0, 1).tolist() == [inf]
        # inf - inf: the default NaN; a signalling NaN: payload kept, quieted, inout first
        assert WR.tree(dt, [_u16(inf), _u16(0x8000 | inf), _u16(ONE[dt])], 3, 0, 0, 1).tolist() == [R.DNAN[dt]]
        sa, sb = inf | 1, 0x8000 | inf | 2
        assert WR.tree(dt, [_u16(sa, ONE[dt]), _u16(sb, sb), _u16(ONE[dt], sa)], 3, 0, 0, 1).tolist() == \
            [sa | q, sb | q]
        assert WR.node(np.array([0x7F800001], np.uint32), np.array([0xFF800002], np.uint32)).tolist() == [0x7FC00001]
        assert WR.node(np.array([0x3F800000], np.uint32), np.array([0xFF800002], np.uint32)).tolist() == [0xFFC00002]
