"""GPU: the derived-target accumulate kernel k_dt_acc_tile (msx_pack.hip) over
every op, element kind and form, byte for byte.

k_dt_acc_tile is what every MPI_Accumulate / MPI_Get_accumulate with a derived
target datatype runs, and path 2 of msx_accumulate_dev.  It is instantiated
once per (op, element kind) of msx_op_kind.h, times REG (the regular layouts'
magic-division map, or the run table's binary search), times ALIGNED (element
loads, or byte copies).

Sections 1-4 run the cases of tests/_dt_acc_cases.py through
test_gpu_accumulate_dev._run: sentinel arenas, the oracle's type map element by
element, oracle.reduce_local / _half_ref.combine, the origin unchanged, and
the library's own pack x 2 -> combine -> unpack sequence as a cross-check.
Every case asserts its plan path first (2; 0 for MPI_NO_OP; 1 for the
one-element targets, see _dt_acc_cases.section3), so none can drift onto the
two-layout kernel.  tests/test_dt_accumulate_cases_cpu.py checks the table
itself.  Section 5 reaches the same kernel through a one-rank window."""
import ctypes
import zlib

import numpy as np
import pytest

import msx
import oracle
import _dt_acc_cases as T
from _cases import h
from oracle import msx_dtype_oracle as O
from test_dtype_cpu import build_oracle, free_all
from test_gpu_accumulate_dev import W, _commit, _data_bytes, _pairs, _run, _same
from test_gpu_batch_local import _data, _esz, _ref

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

C = msx.C
c_int = ctypes.c_int


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    lib = msx.init(errors_return=True)
    assert lib.msx_device_count() > 0
    return lib


def _go(L, c):
    args, kw = T.run_args(c)
    plan = _run(L, *args, **kw)
    if c.op != "MPI_NO_OP":
        assert plan[2] == _esz(c.edt), (c.id, plan)


# ---- 1. every (op, element kind) in all four forms -----------------------------------

@pytest.mark.parametrize("pair", _pairs(), ids=lambda p: f"{p[0]}-{p[1]}")
def test_every_op_and_element_kind_in_all_four_forms(L, pair):
    """W + 1 elements through vector(W+1, 1, 3) (regular) and 266 through 19
    instances of five uneven blocks (table), each with aligned pointers and
    with the packed stream 1 byte and the typed base 3 bytes off 16-byte
    alignment (the byte-copy form).  1-byte kinds have alignof(T) = 1, so no
    unaligned form exists for them and only the two aligned cases run.  The
    pair datatypes (MPI_FLOAT_INT ...) have no single element type and are
    refused by the plan, as _pairs() documents."""
    for c in T.pair_cases(pair):
        _go(L, c)


# ---- 2. operand order, directed ------------------------------------------------------

@pytest.mark.parametrize("entry", T.DIRECTED, ids=lambda e: f"{e[0]}-{e[1]}")
def test_operand_order_on_the_full_cross_product_of_edge_values(L, entry):
    """target (op)= origin, in that order: the ordered cross product of 15
    edge values (two NaNs of either sign with payloads of their own against
    each other, +0 against -0, ties for MAXLOC / MINLOC with the locations in
    both orders) leads the operands of all four forms.  Fn<OP>::apply(in,
    inout) instead of (inout, in) changes which NaN, which zero and which
    location survives."""
    for c in T.directed_cases(entry):
        _go(L, c)


# ---- 3. tile edges -------------------------------------------------------------------

@pytest.mark.parametrize("c", T.section3(), ids=lambda c: c.id)
def test_element_counts_around_the_wave_and_the_tile(L, c):
    _go(L, c)


# ---- 4. layout forms -----------------------------------------------------------------

@pytest.mark.parametrize("c", T.section4(), ids=lambda c: c.id)
def test_layout_forms(L, c):
    """_dt_acc_cases.layouts names which recipe reaches which form."""
    _go(L, c)


# ---- 5. the same kernel through a window ---------------------------------------------
# MPI_Accumulate / MPI_Get_accumulate on this rank's own window apply at once
# (rma_apply_typed -> dt_acc_dev): a device window in place, a pageable host
# window staged through HBM at the same offset from 16-byte alignment.

WIN_BYTES = 16 << 10
PAT_W = 0xA5
# one datatype per element size; the ops of the six families that are legal for it
WIN_TYPES = ("MPI_INT8_T", "MPI_UINT16_T", "MPI_FLOAT", "MPI_DOUBLE", "MPI_2DOUBLE_PRECISION")
WIN_OPS = ("MPI_SUM", "MPI_PROD", "MPI_MAX", "MPI_LXOR", "MPI_BOR", "MPI_MAXLOC")


def _win_layouts(e):
    return [(("vector", W + 1, 1, 3, e), 1),
            (T.IX(e), T.IX_COUNT),
            (("subarray", [7, 9, 11], [5, 6, 9], [1, 2, 1], True, e), 1),
            (("vector", 1, 1, 3, e), 1)]               # one element: the kernel's smallest launch


class _Window:
    """WIN_BYTES of window memory: on the device, in pageable host memory on a
    16-byte boundary, or one byte past one (a numpy slice)."""

    def __init__(self, kind):
        self.kind = kind
        if kind == "device":
            self.t = torch.empty(WIN_BYTES, dtype=torch.uint8, device="cuda")
            self.ptr = self.t.data_ptr()
            assert self.ptr % 16 == 0
        else:
            self.buf = np.empty(WIN_BYTES + 32, np.uint8)
            off = -self.buf.ctypes.data % 16 + (1 if kind == "host+1" else 0)
            self.v = self.buf[off:off + WIN_BYTES]
            self.ptr = self.v.ctypes.data
            assert self.ptr % 16 == (1 if kind == "host+1" else 0)

    def write(self, img):
        if self.kind == "device":
            self.t.copy_(torch.from_numpy(img))
            torch.cuda.synchronize()
        else:
            self.v[:] = img

    def read(self):
        torch.cuda.synchronize()
        return self.t.cpu().numpy() if self.kind == "device" else self.v.copy()


def _operand(data, on_device, off=0):
    """`data` bytes as a call's origin: (keep-alive, address); a device copy
    may sit `off` bytes past 16-byte alignment."""
    if on_device:
        t = torch.empty(data.size + 16, dtype=torch.uint8, device="cuda")
        t[off:off + data.size] = torch.from_numpy(data.copy())
        torch.cuda.synchronize()
        return t, t.data_ptr() + off
    a = data.copy()
    return a, a.ctypes.data


@pytest.mark.parametrize("kind", ["device", "host", "host+1"])
def test_accumulate_and_get_accumulate_through_a_one_rank_window(L, kind):
    """Predefined origins (device, device one byte off alignment, pageable
    host) into derived targets at a nonzero target_disp.  After every call the
    whole window equals the oracle's image (unmapped bytes unchanged); the
    fetched values are the pre-op ones in type-map order; MPI_NO_OP fetches
    and changes nothing.  In the host+1 window every typed address is off the
    element alignment, which the HBM staging keeps: the byte-copy form."""
    w = _Window(kind)
    win = c_int()
    assert L.MPI_Win_create(ctypes.c_void_p(w.ptr), WIN_BYTES, 1, C.MPI_INFO_NULL, C.MPI_COMM_WORLD,
                            ctypes.byref(win)) == 0, msx.last_error()
    assert L.MPI_Win_set_errhandler(win, C.MPI_ERRORS_RETURN) == 0
    assert L.MPI_Win_fence(0, win) == 0
    step = 0
    for dt in WIN_TYPES:
        esz, e = _esz(dt), T.E(dt)
        ops = [op for op in WIN_OPS if oracle.op_check(h(op), h(dt)) == 0]
        assert ops, dt
        for trec, tcount in _win_layouts(e):
            keep = []
            th = _commit(L, trec, keep)
            tt = build_oracle(trec)
            disp = 3 * esz + 64
            lo, hi = O.span(tt, tcount)
            assert disp + lo >= 0 and disp + hi <= WIN_BYTES
            tb = _data_bytes(tt, tcount, disp)
            n = tb.size // esz
            for op in ops + ["MPI_NO_OP"]:
                step += 1
                tag = f"{kind} {op} {dt} {trec[0]} x{tcount}"
                rng = np.random.default_rng(zlib.crc32(f"win/{kind}/{op}/{dt}/{trec[0]}/{n}".encode()))
                dop = "MPI_SUM" if op == "MPI_NO_OP" else op
                img = np.full(WIN_BYTES, PAT_W, np.uint8)
                img[tb] = _data(dop, dt, n, rng)
                w.write(img)
                org, org2 = _data(dop, dt, n, rng), _data(dop, dt, n, rng)
                exp = img.copy()
                if op != "MPI_NO_OP":
                    # MPI_Accumulate, the origin's place changing from call to call
                    hold, optr = _operand(org, step % 3 != 0, step % 2 if esz > 1 else 0)
                    assert L.MPI_Accumulate(ctypes.c_void_p(optr), n, h(dt), 0, disp, tcount, th, h(op),
                                            win) == 0, (tag, msx.last_error())
                    assert L.MPI_Win_fence(0, win) == 0, msx.last_error()
                    exp[tb] = _ref(op, dt, org, img[tb])
                    _same(w.read(), exp, tag + " accumulate")
                # MPI_Get_accumulate on what the window holds now
                hold2, optr2 = _operand(org2, step % 3 != 1, (step + 1) % 2 if esz > 1 else 0)
                res_dev = step % 2 == 0
                res = (torch.zeros(n * esz, dtype=torch.uint8, device="cuda") if res_dev
                       else np.zeros(n * esz, np.uint8))
                torch.cuda.synchronize()
                rptr = res.data_ptr() if res_dev else res.ctypes.data
                assert L.MPI_Get_accumulate(ctypes.c_void_p(optr2), n, h(dt), ctypes.c_void_p(rptr), n, h(dt), 0, disp,
                                            tcount, th, h(op), win) == 0, (tag, msx.last_error())
                assert L.MPI_Win_fence(0, win) == 0, msx.last_error()
                torch.cuda.synchronize()
                got_res = res.cpu().numpy() if res_dev else res
                assert np.array_equal(got_res, exp[tb]), tag + ": fetched values"
                exp2 = exp.copy()
                if op != "MPI_NO_OP":
                    exp2[tb] = _ref(op, dt, org2, exp[tb])
                _same(w.read(), exp2, tag + " get_accumulate")
            free_all(L, keep)
    assert L.MPI_Win_free(ctypes.byref(win)) == 0
