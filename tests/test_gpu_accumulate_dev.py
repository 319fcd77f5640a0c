"""GPU: msx_accumulate_dev (the two-layout kernels of msx_acc2.hip and the three
existing paths it forwards to) against an independent numpy reference, byte for
byte.

The reference takes the two type maps from oracle/msx_dtype_oracle.py (element
by element, not the library's merged runs), gathers the origin's elements and
the first n of the target's, combines them with the oracle's op.cpp restatement
(_half_ref.combine for the 16-bit floats) and scatters the result.  Both
operands live in arenas filled with a sentinel, 64 guard bytes at either end;
after every call the whole target arena must equal the expected image (so every
unmapped byte kept its sentinel) and the whole origin arena must be unchanged.
For every op case the same inputs also go through the library's own
msx_pack_dev x 2 -> msx_reduce_local_dev -> msx_unpack_dev sequence, which must
give the same arena.  The plan (msx_accumulate_plan) is asserted before every
call, so each case is known to run the path it is meant for."""
import ctypes
import zlib

import numpy as np
import pytest

import msx
import oracle
import _half_ref as R
from oracle import msx_dtype_oracle as O
from _cases import KIND, h, legal_pairs
from test_dtype_cpu import build_lib, build_oracle, free_all
from test_gpu_batch_local import _data, _esz, _ref

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

C = msx.C
i64, c_int = ctypes.c_int64, ctypes.c_int
GUARD = 64
PAT_O, PAT_T = 0x5A, 0xA5
W = 256                      # elements per workgroup of the two-layout kernels (kUnroll x 64)
PAIR_TYPES = ("MPI_FLOAT_INT", "MPI_DOUBLE_INT", "MPI_LONG_INT", "MPI_SHORT_INT", "MPI_LONG_DOUBLE_INT")


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    lib = msx.init(errors_return=True)
    assert lib.msx_device_count() > 0
    return lib


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _commit(L, r, keep):
    if r[0] == "basic":
        return r[1]
    x = c_int(build_lib(L, r, keep))
    assert L.MPI_Type_commit(ctypes.byref(x)) == 0
    return x.value


def _plan(L, oc, odt, tc, tdt, op):
    n, path, gran = i64(-7), c_int(-7), c_int(-7)
    rc = L.msx_accumulate_plan(oc, odt, tc, tdt, op, ctypes.byref(n), ctypes.byref(path), ctypes.byref(gran))
    assert rc == 0, msx.last_error()
    return n.value, path.value, gran.value


def _data_bytes(t, count, base):
    """Arena index of every data byte of `count` instances, in type-map order."""
    d = np.concatenate([np.arange(x, x + s) for x, s in t.typemap]).astype(np.int64)
    return (base + np.arange(count, dtype=np.int64)[:, None] * t.extent + d[None, :]).ravel()


def _arena(t, count, mis, pat):
    """A sentinel-filled arena for `count` instances whose buffer address sits
    `mis` bytes off 16-byte alignment: (image, index of the buffer address)."""
    lo, hi = O.span(t, count)
    base = GUARD - lo + mis
    base += -(base - mis) % 16
    return np.full(base + hi + GUARD + 16, pat, np.uint8), base


def _up(img):
    t = torch.from_numpy(img.copy()).pin_memory().cuda()
    assert t.data_ptr() % 16 == 0
    return t


def _same(got, exp, tag):
    if np.array_equal(got, exp):
        return
    i = int(np.nonzero(got != exp)[0][0])
    pytest.fail(f"{tag}: {int((got != exp).sum())} bytes differ, first at arena byte {i}: "
                f"got {int(got[i]):#04x} exp {int(exp[i]):#04x}")


def _run(L, op, dt, orec, ocount, trec, tcount, path, mis_o=0, mis_t=0, seed=0, data=None):
    """One msx_accumulate_dev call checked as the module docstring says.
    dt: the element datatype's name for an op, None for MPI_REPLACE / MPI_NO_OP
    (random bytes).  data: the (origin, target) data bytes in type-map order for
    a directed case, instead of _data's.  Returns the plan."""
    keep = []
    oh, th = _commit(L, orec, keep), _commit(L, trec, keep)
    ot, tt = build_oracle(orec), build_oracle(trec)
    rng = np.random.default_rng(zlib.crc32(f"acc2/{op}/{dt}/{seed}/{ocount}/{tcount}".encode()))
    img_o, bo = _arena(ot, ocount, mis_o, PAT_O)
    img_t, bt = _arena(tt, tcount, mis_t, PAT_T)
    ob, tb = _data_bytes(ot, ocount, bo), _data_bytes(tt, tcount, bt)
    nb = ob.size
    assert nb <= tb.size and len(set(tb.tolist())) == tb.size          # a legal target map
    if data is not None:
        assert data[0].size == nb and data[1].size == tb.size
        img_o[ob], img_t[tb] = data
    elif dt is None:
        img_o[ob] = rng.integers(0, 256, nb, dtype=np.uint8)
        img_t[tb] = rng.integers(0, 256, tb.size, dtype=np.uint8)
    else:
        esz = _esz(dt)
        assert nb % esz == 0 and tb.size % esz == 0
        img_o[ob] = _data(op, dt, nb // esz, rng)
        img_t[tb] = _data(op, dt, tb.size // esz, rng)
    exp = img_t.copy()
    if op == "MPI_REPLACE":
        exp[tb[:nb]] = img_o[ob]
    elif op != "MPI_NO_OP":
        exp[tb[:nb]] = _ref(op, dt, img_o[ob], img_t[tb[:nb]])
    plan = _plan(L, ocount, oh, tcount, th, h(op))
    assert plan[0] == len(ot.typemap) * ocount
    assert plan[1] == path, (plan, orec, trec)
    d_o, d_t = _up(img_o), _up(img_t)
    torch.cuda.synchronize()
    rc = L.msx_accumulate_dev(d_o.data_ptr() + bo, ocount, oh, d_t.data_ptr() + bt, tcount, th, h(op), _stream())
    assert rc == 0, msx.last_error()
    torch.cuda.synchronize()
    tag = f"{op} {dt} {orec} x{ocount} -> {trec} x{tcount}"
    got = d_t.cpu().numpy()
    _same(got, exp, tag)
    assert np.array_equal(d_o.cpu().numpy(), img_o), f"{tag}: the origin arena changed"
    if dt is not None:
        _same(got, _by_public_sequence(L, op, dt, img_o, bo, oh, ocount, img_t, bt, th, tcount, nb), tag + " vs sequence")
    free_all(L, keep)
    return plan


def _by_public_sequence(L, op, dt, img_o, bo, oh, ocount, img_t, bt, th, tcount, nb):
    """The four launches the call replaces, on copies of the same arenas."""
    d_o, d_t = _up(img_o), _up(img_t)
    tsize = c_int()
    assert L.MPI_Type_size(th, ctypes.byref(tsize)) == 0
    po = torch.empty(nb, dtype=torch.uint8, device="cuda")
    pt = torch.empty(tcount * tsize.value, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s = _stream()
    assert L.msx_pack_dev(d_o.data_ptr() + bo, ocount, oh, po.data_ptr(), s) == 0, msx.last_error()
    assert L.msx_pack_dev(d_t.data_ptr() + bt, tcount, th, pt.data_ptr(), s) == 0, msx.last_error()
    assert L.msx_reduce_local_dev(po.data_ptr(), pt.data_ptr(), nb // _esz(dt), h(dt), h(op), s) == 0, msx.last_error()
    assert L.msx_unpack_dev(pt.data_ptr(), tcount, th, d_t.data_ptr() + bt, s) == 0, msx.last_error()
    torch.cuda.synchronize()
    return d_t.cpu().numpy()


F = ("basic", C.MPI_FLOAT)
IX = ("indexed", [3, 1, 4, 1, 5], [0, 5, 7, 13, 16], F)          # 14 elements in 5 uneven blocks
IX2 = ("indexed", [5, 1, 4, 1, 3], [1, 8, 10, 15, 17], F)


# ---- regular layouts ---------------------------------------------------------------

@pytest.mark.parametrize("count", [1, 7])
def test_vector_into_vector(L, count):
    """MPI_Type_vector(37, 1, 5) -> (37, 1, 3) on fp32: one instance, and seven
    (259 elements: a second workgroup with three live lanes)."""
    _run(L, "MPI_SUM", "MPI_FLOAT", ("vector", 37, 1, 5, F), count, ("vector", 37, 1, 3, F), count, 4)


@pytest.mark.parametrize("n", [W - 1, W, W + 1, 3 * W + 5])
def test_element_counts_around_the_workgroup(L, n):
    _run(L, "MPI_SUM", "MPI_FLOAT", ("vector", n, 1, 5, F), 1, ("vector", n, 1, 3, F), 1, 4)
    _run(L, "MPI_REPLACE", None, ("vector", n, 1, 5, F), 1, ("vector", n, 1, 3, F), 1, 4)


@pytest.mark.parametrize("order_c", [True, False], ids=["C", "Fortran"])
def test_subarray_into_a_subarray_of_another_shape(L, order_c):
    """Two-level layouts on both sides: sub (3,4,5) of (6,7,8) into sub (5,6,2)
    of (7,9,4), 60 elements each; five instances make 300."""
    o = ("subarray", [6, 7, 8], [3, 4, 5], [2, 1, 3], order_c, F)
    t = ("subarray", [7, 9, 4], [5, 6, 2], [1, 3, 1], order_c, F)
    for count in (1, 5):
        _run(L, "MPI_SUM", "MPI_FLOAT", o, count, t, count, 4)
    _run(L, "MPI_REPLACE", None, o, 5, t, 5, 4)


# ---- irregular layouts -------------------------------------------------------------

@pytest.mark.parametrize("pair", [(IX, ("vector", 14, 1, 2, F)), (("vector", 14, 1, 2, F), IX), (IX, IX2)],
                         ids=["indexed-vector", "vector-indexed", "indexed-indexed"])
def test_indexed_layouts(L, pair):
    """The run tables' binary search on either side and on both; 20 instances
    are 280 elements."""
    for count in (1, 20):
        _run(L, "MPI_SUM", "MPI_FLOAT", pair[0], count, pair[1], count, 4)
    _run(L, "MPI_REPLACE", None, pair[0], 20, pair[1], 20, 4)


# ---- counts, extents, coverage -----------------------------------------------------

def test_unequal_counts_with_resized_extents(L):
    """6 x 10 elements into 4 x 15: the instance boundaries of the two sides
    fall at different elements.  Then a negative-stride hvector with a negative
    lb as the origin, and as the target."""
    o = ("resized", 0, 100, ("vector", 10, 1, 2, F))
    t = ("resized", 0, 200, ("vector", 15, 1, 3, F))
    _run(L, "MPI_SUM", "MPI_FLOAT", o, 6, t, 4, 4)
    neg = ("resized", -16, 136, ("hvector", 10, 1, -12, F))
    _run(L, "MPI_SUM", "MPI_FLOAT", neg, 6, t, 4, 4)
    _run(L, "MPI_SUM", "MPI_FLOAT", o, 6, ("resized", -16, 208, ("hvector", 15, 1, -12, F)), 4, 4)
    _run(L, "MPI_REPLACE", None, neg, 30, t, 20, 4)


def test_partial_coverage_of_the_last_target_instance(L):
    """50 origin elements into a 60-element target type: the last 10 mapped
    target elements keep their values."""
    _run(L, "MPI_SUM", "MPI_FLOAT", ("vector", 50, 1, 2, F), 1, ("vector", 60, 1, 3, F), 1, 4)
    _run(L, "MPI_MAX", "MPI_DOUBLE", ("vector", 50, 1, 2, ("basic", C.MPI_DOUBLE)), 7,
         ("vector", 60, 1, 3, ("basic", C.MPI_DOUBLE)), 6, 4)           # 350 into 360
    _run(L, "MPI_REPLACE", None, ("vector", 50, 1, 2, F), 1, ("vector", 60, 1, 3, F), 1, 4)


# ---- the unaligned form ------------------------------------------------------------

@pytest.mark.parametrize("mis", [(1, 0), (0, 1), (1, 1), (3, 2)], ids=lambda m: f"o{m[0]}t{m[1]}")
def test_base_pointers_off_the_element_alignment(L, mis):
    _run(L, "MPI_SUM", "MPI_FLOAT", ("vector", W + 1, 1, 5, F), 1, ("vector", W + 1, 1, 3, F), 1, 4, *mis)
    _run(L, "MPI_SUM", "MPI_DOUBLE", ("vector", 40, 1, 5, ("basic", C.MPI_DOUBLE)), 1,
         ("vector", 40, 1, 3, ("basic", C.MPI_DOUBLE)), 1, 4, 4 * mis[0], 4 * mis[1])


def test_hindexed_with_odd_byte_displacements(L):
    odd = ("hindexed", [2, 1, 3], [1, 15, 29], F)
    _run(L, "MPI_SUM", "MPI_FLOAT", odd, 50, ("vector", 6, 1, 2, F), 50, 4)
    _run(L, "MPI_SUM", "MPI_FLOAT", ("vector", 6, 1, 2, F), 50, odd, 50, 4)
    _run(L, "MPI_PROD", "MPI_FLOAT", odd, 50, ("hindexed", [3, 3], [3, 21], F), 50, 4)
    _run(L, "MPI_REPLACE", None, odd, 50, ("vector", 6, 1, 2, F), 50, 4)


# ---- every (op, element kind) pair --------------------------------------------------

def _pairs():
    """One datatype per (op, element kind) of the accumulate's map.  The pair
    types (MPI_FLOAT_INT ...) have no single basic element type, so the kinds
    only they name (fi, si, di) cannot reach the combine: check 6 refuses them
    (tests/test_accumulate_dev_cpu.py)."""
    seen, out = set(), []
    for op, dt in legal_pairs(oracle):
        if dt in PAIR_TYPES or (op, KIND[dt]) in seen:
            continue
        seen.add((op, KIND[dt]))
        out.append((op, dt))
    return out + [(op, dt) for dt in R.TYPES for op in R.OPS]


@pytest.mark.parametrize("pair", _pairs(), ids=lambda p: f"{p[0]}-{p[1]}")
def test_every_op_and_element_kind(L, pair):
    """W + 1 elements through the two-layout kernel with the edge-value
    operands of _cases.gen: element sizes 1, 2, 4, 8 and 16."""
    op, dt = pair
    e = ("basic", h(dt))
    _run(L, op, dt, ("vector", W + 1, 1, 2, e), 1, ("vector", W + 1, 1, 3, e), 1, 4)


def test_the_sweep_covers_every_element_size():
    assert {_esz(dt) for _, dt in _pairs()} == {1, 2, 4, 8, 16}
    assert len(_pairs()) >= 100


# ---- MPI_REPLACE and MPI_NO_OP -------------------------------------------------------

@pytest.mark.parametrize("G", [1, 2, 4, 8, 16])
def test_replace_at_each_granule(L, G):
    b = ("basic", C.MPI_BYTE)
    o, t = ("vector", 37, G, 3 * G, b), ("vector", 37, G, 5 * G, b)
    assert _run(L, "MPI_REPLACE", None, o, 9, t, 9, 4)[2] == G
    # the pointers count as well: 16-byte blocks at a 4-byte offset move in 4-byte granules
    if G == 16:
        _run(L, "MPI_REPLACE", None, o, 9, t, 9, 4, 4, 8)


def test_replace_between_mixed_structs(L):
    i8, f8 = ("basic", C.MPI_INT8_T), ("basic", C.MPI_DOUBLE)
    o = ("struct", [1, 1], [0, 8], [i8, f8])
    t = ("struct", [1, 1], [16, 0], [i8, f8])
    assert _run(L, "MPI_REPLACE", None, o, 40, t, 40, 4)[2] == 1
    _run(L, "MPI_REPLACE", None, o, 40, ("vector", 90, 1, 2, F), 1, 4)


def test_no_op_writes_nothing(L):
    assert _run(L, "MPI_NO_OP", None, ("vector", 37, 1, 5, F), 3, ("vector", 37, 1, 3, F), 3, 0)[0] == 111


# ---- the paths that forward to existing kernels --------------------------------------

def test_both_sides_contiguous_is_msx_reduce_local_dev(L):
    for n in (1, 1000, 4099):
        _run(L, "MPI_SUM", "MPI_FLOAT", F, n, F, n, 1)
    _run(L, "MPI_SUM", "MPI_FLOAT", ("contig", 10, F), 30, F, 400, 1)
    _run(L, "MPI_MAXLOC", "MPI_2INT", ("basic", C.MPI_2INT), 300, ("contig", 3, ("basic", C.MPI_2INT)), 100, 1)
    _run(L, "MPI_REPLACE", None, F, 1000, ("contig", 10, F), 100, 1)
    _run(L, "MPI_SUM", "MPI_FLOAT", F, 3, ("vector", 5, 4, 6, F), 1, 1)      # inside the target's first run


def test_contiguous_origin_is_the_derived_target_accumulate(L):
    _run(L, "MPI_SUM", "MPI_FLOAT", F, 111, ("vector", 37, 1, 3, F), 3, 2)
    _run(L, "MPI_MIN", "MPI_FLOAT", ("contig", 14, F), 20, IX, 25, 2)
    _run(L, "MPI_REPLACE", None, F, 111, ("vector", 37, 1, 3, F), 3, 2)


def test_replace_into_a_contiguous_target_is_the_pack(L):
    _run(L, "MPI_REPLACE", None, ("vector", 37, 1, 5, F), 3, F, 111, 3)
    _run(L, "MPI_REPLACE", None, IX, 20, ("contig", 7, F), 50, 3)
    _run(L, "MPI_SUM", "MPI_FLOAT", ("vector", 37, 1, 5, F), 3, F, 111, 4)   # an op has no such kernel


# ---- overlapping spans, stream order -------------------------------------------------

def test_column_into_column_of_one_matrix(L):
    """Column j += column k of one 300 x 7 fp32 matrix: the two spans interleave
    element by element."""
    rows, cols, j, k = 300, 7, 2, 5
    keep = []
    col = _commit(L, ("vector", rows, 1, cols, F), keep)
    rng = np.random.default_rng(7)
    m = rng.uniform(-4, 4, (rows, cols)).astype(np.float32)
    exp = m.copy()
    a, b = np.ascontiguousarray(m[:, k]), np.ascontiguousarray(m[:, j])
    assert oracle.reduce_local(C.MPI_SUM, C.MPI_FLOAT, a, b) == 0
    exp[:, j] = b
    d = torch.from_numpy(m.copy()).cuda()
    assert _plan(L, 1, col, 1, col, C.MPI_SUM) == (rows, 4, 4)
    torch.cuda.synchronize()
    rc = L.msx_accumulate_dev(d.data_ptr() + 4 * k, 1, col, d.data_ptr() + 4 * j, 1, col, C.MPI_SUM, _stream())
    assert rc == 0, msx.last_error()
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy().view(np.uint32), exp.view(np.uint32))
    free_all(L, keep)


def test_stream_order(L):
    """On a non-default stream: a copy that writes the origin, the call, and the
    readback, all enqueued on that stream with no host synchronisation between
    them; only the stream is synchronised before the check."""
    n = 3 * W + 5
    keep = []
    oh, th = _commit(L, ("vector", n, 1, 5, F), keep), _commit(L, ("vector", n, 1, 3, F), keep)
    rng = np.random.default_rng(11)
    a, b = rng.uniform(-4, 4, (n, 5)).astype(np.float32), rng.uniform(-4, 4, (n, 3)).astype(np.float32)
    exp = b.copy()
    col = np.ascontiguousarray(b[:, 0])
    assert oracle.reduce_local(C.MPI_SUM, C.MPI_FLOAT, np.ascontiguousarray(a[:, 0]), col) == 0
    exp[:, 0] = col
    d_o = torch.zeros(n, 5, dtype=torch.float32, device="cuda")            # not the origin yet
    d_t = torch.from_numpy(b.copy()).cuda()
    src = torch.from_numpy(a.copy()).pin_memory()
    back = torch.empty(n, 3, dtype=torch.float32).pin_memory()
    assert _plan(L, 1, oh, 1, th, C.MPI_SUM) == (n, 4, 4)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_o.copy_(src, non_blocking=True)
        rc = L.msx_accumulate_dev(d_o.data_ptr(), 1, oh, d_t.data_ptr(), 1, th, C.MPI_SUM,
                                  ctypes.c_void_p(s.cuda_stream))
        back.copy_(d_t, non_blocking=True)
    assert rc == 0, msx.last_error()
    s.synchronize()
    assert np.array_equal(back.numpy().view(np.uint32), exp.view(np.uint32))
    free_all(L, keep)


# ---- 2^32 elements and more: the 64-bit address map ----------------------------------

@pytest.mark.parametrize("op", ["MPI_SUM", "MPI_REPLACE"])
def test_more_than_4_gi_elements(L, op):
    """2049 instances of two 1 MiB rows of int8, 2^32 + 2^21 elements: the
    element index no longer fits the 32-bit divisions.  Rows of 1 MiB + 16 bytes
    into rows of 1 MiB + 48 bytes; torch computes the reference on the GPU.
    MPI_REPLACE runs from an origin one byte off alignment, so it moves single
    bytes and its granule index passes 2^32 as well."""
    row, po, pt, inst = 1 << 20, 16, 48, 2049
    i8 = ("basic", C.MPI_INT8_T)
    keep = []
    oh = _commit(L, ("resized", 0, 2 * (row + po), ("vector", 2, row, row + po, i8)), keep)
    th = _commit(L, ("resized", 0, 2 * (row + pt), ("vector", 2, row, row + pt, i8)), keep)
    mis = 1 if op == "MPI_REPLACE" else 0
    g = torch.Generator(device="cuda").manual_seed(5)
    d_o = torch.randint(-128, 128, (2 * inst * (row + po) + 16,), dtype=torch.int8, device="cuda", generator=g)
    d_t = torch.randint(-128, 128, (2 * inst, row + pt), dtype=torch.int8, device="cuda", generator=g)
    ov = d_o[mis:mis + 2 * inst * (row + po)].view(2 * inst, row + po)
    o_before = d_o.clone()
    exp = d_t.clone()
    exp[:, :row] = ov[:, :row] if op == "MPI_REPLACE" else exp[:, :row] + ov[:, :row]      # int8 wraps
    n, path, gran = _plan(L, inst, oh, inst, th, h(op))
    assert (n, path) == (2 * inst * row, 4) and n > 1 << 32
    torch.cuda.synchronize()
    rc = L.msx_accumulate_dev(d_o.data_ptr() + mis, inst, oh, d_t.data_ptr(), inst, th, h(op), _stream())
    assert rc == 0, msx.last_error()
    torch.cuda.synchronize()
    assert torch.equal(d_t, exp)
    assert torch.equal(d_o, o_before)
    free_all(L, keep)
