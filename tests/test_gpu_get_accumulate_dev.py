"""GPU: msx_get_accumulate_dev (the three-layout kernels of msx_acc3.hip, the
fetch kernel of msx_fetch.hip on contiguous pieces, and the typed -> typed copy
MPI_NO_OP forwards to) against an independent numpy reference, byte for byte.

The reference takes the three type maps from oracle/msx_dtype_oracle.py (element
by element), gathers the first n elements of the origin and of the target,
combines them with the oracle's op.cpp restatement (_half_ref.combine for the
16-bit floats), scatters the combine into the target and the target's old
elements into the result.  The three operands live in arenas filled with a
sentinel, 64 guard bytes at either end; after every call the whole target and
result arenas must equal the expected images (every unmapped byte, and every
mapped byte past n, kept) and the whole origin arena must be unchanged.  For
every op case the same inputs also go through the library's own two calls,
msx_accumulate_dev(MPI_REPLACE, target -> result) then msx_accumulate_dev(op,
origin -> target), which must give the same two arenas.  The plan
(msx_get_accumulate_plan) is asserted before every call, so each case is known
to run the path it is meant for."""
import ctypes
import zlib

import numpy as np
import pytest

import msx
import oracle
from _cases import h
from test_dtype_cpu import build_oracle, free_all
from test_gpu_accumulate_dev import W, _arena, _commit, _data_bytes, _same, _up
from test_gpu_batch_local import _data, _esz, _ref

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

C = msx.C
i64, c_int = ctypes.c_int64, ctypes.c_int
PAT_O, PAT_R, PAT_T = 0x5A, 0xC3, 0xA5


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    lib = msx.init(errors_return=True)
    assert lib.msx_device_count() > 0
    return lib


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _plan(L, oc, odt, rc_, rdt, tc, tdt, op):
    n, path, gran = i64(-7), c_int(-7), c_int(-7)
    rc = L.msx_get_accumulate_plan(oc, odt, rc_, rdt, tc, tdt, op, ctypes.byref(n), ctypes.byref(path),
                                   ctypes.byref(gran))
    assert rc == 0, msx.last_error()
    return n.value, path.value, gran.value


def _run(L, op, dt, orec, ocount, rrec, rcount, trec, tcount, path, mis=(0, 0, 0), tprefix=None, seed=0):
    """One msx_get_accumulate_dev call checked as the module docstring says.
    dt: the element datatype's name for an op, None for MPI_REPLACE / MPI_NO_OP
    (random bytes).  Under MPI_NO_OP the origin triple is (NULL, 0, 0) and orec
    is ignored.  tprefix: (recipe, count) naming exactly the first n elements of
    the target, for the two-call sequence when n ends inside a target instance.
    Returns the plan."""
    noop = op == "MPI_NO_OP"
    keep = []
    rh, th = _commit(L, rrec, keep), _commit(L, trec, keep)
    rt, tt = build_oracle(rrec), build_oracle(trec)
    oh, ot = (0, None) if noop else (_commit(L, orec, keep), build_oracle(orec))
    rng = np.random.default_rng(zlib.crc32(f"acc3/{op}/{dt}/{seed}/{ocount}/{rcount}/{tcount}".encode()))
    img_r, br = _arena(rt, rcount, mis[1], PAT_R)
    img_t, bt = _arena(tt, tcount, mis[2], PAT_T)
    rb, tb = _data_bytes(rt, rcount, br), _data_bytes(tt, tcount, bt)
    if noop:
        img_o, bo, ob = np.full(16, PAT_O, np.uint8), 0, None
        nb, nel = rb.size, len(rt.typemap) * rcount
    else:
        img_o, bo = _arena(ot, ocount, mis[0], PAT_O)
        ob = _data_bytes(ot, ocount, bo)
        nb, nel = ob.size, len(ot.typemap) * ocount
    assert nb <= tb.size and nb <= rb.size
    assert len(set(tb.tolist())) == tb.size and len(set(rb.tolist())) == rb.size      # legal target and result maps
    img_r[rb] = rng.integers(0, 256, rb.size, dtype=np.uint8)
    if dt is None:
        if not noop:
            img_o[ob] = rng.integers(0, 256, nb, dtype=np.uint8)
        img_t[tb] = rng.integers(0, 256, tb.size, dtype=np.uint8)
    else:
        esz = _esz(dt)
        assert nb % esz == 0 and tb.size % esz == 0
        img_o[ob] = _data(op, dt, nb // esz, rng)
        img_t[tb] = _data(op, dt, tb.size // esz, rng)
    exp_r, exp_t = img_r.copy(), img_t.copy()
    exp_r[rb[:nb]] = img_t[tb[:nb]]
    if op == "MPI_REPLACE":
        exp_t[tb[:nb]] = img_o[ob]
    elif not noop:
        exp_t[tb[:nb]] = _ref(op, dt, img_o[ob], img_t[tb[:nb]])
    plan = _plan(L, ocount, oh, rcount, rh, tcount, th, h(op))
    assert plan[0] == nel
    assert plan[1] == path, (plan, orec, rrec, trec)
    d_o, d_r, d_t = _up(img_o), _up(img_r), _up(img_t)
    torch.cuda.synchronize()
    origin = None if noop else d_o.data_ptr() + bo
    rc = L.msx_get_accumulate_dev(origin, ocount, oh, d_r.data_ptr() + br, rcount, rh, d_t.data_ptr() + bt, tcount, th,
                                  h(op), _stream())
    assert rc == 0, msx.last_error()
    torch.cuda.synchronize()
    tag = f"{op} {dt} {orec} x{ocount} / {rrec} x{rcount} / {trec} x{tcount}"
    got_r, got_t = d_r.cpu().numpy(), d_t.cpu().numpy()
    _same(got_t, exp_t, tag + " target")
    _same(got_r, exp_r, tag + " result")
    assert np.array_equal(d_o.cpu().numpy(), img_o), f"{tag}: the origin arena changed"
    if dt is not None:
        # the library's own two calls on fresh copies of the same arenas
        if tprefix is None:
            assert nb % tt.size == 0
            ph, pcount = th, nb // tt.size
        else:
            ph, pcount = _commit(L, tprefix[0], keep), tprefix[1]
            pt = build_oracle(tprefix[0])
            assert np.array_equal(_data_bytes(pt, pcount, bt), tb[:nb])
        e_o, e_r, e_t = _up(img_o), _up(img_r), _up(img_t)
        torch.cuda.synchronize()
        s = _stream()
        assert L.msx_accumulate_dev(e_t.data_ptr() + bt, pcount, ph, e_r.data_ptr() + br, rcount, rh, C.MPI_REPLACE,
                                    s) == 0, msx.last_error()
        assert L.msx_accumulate_dev(e_o.data_ptr() + bo, ocount, oh, e_t.data_ptr() + bt, tcount, th, h(op),
                                    s) == 0, msx.last_error()
        torch.cuda.synchronize()
        _same(got_t, e_t.cpu().numpy(), tag + " target vs the two calls")
        _same(got_r, e_r.cpu().numpy(), tag + " result vs the two calls")
    free_all(L, keep)
    return plan


F = ("basic", C.MPI_FLOAT)
D = ("basic", C.MPI_DOUBLE)
IX = ("indexed", [3, 1, 4, 1, 5], [0, 5, 7, 13, 16], F)          # 14 elements in 5 uneven blocks
IX2 = ("indexed", [5, 1, 4, 1, 3], [1, 8, 10, 15, 17], F)
IX3 = ("indexed", [2, 6, 1, 5], [0, 3, 10, 12], F)
SUB2 = ("subarray", [9, 8], [5, 6], [2, 1], True, F)             # 30 elements in rows of 6
SUB3 = ("subarray", [6, 7, 8], [3, 4, 5], [2, 1, 3], True, F)    # 60 elements in rows of 5
V16 = ("vector", 105, 4, 8, F)                                    # 420 elements: 16-byte blocks at a 32-byte stride
V1 = ("vector", 420, 1, 3, F)                                     # one-element blocks

# 420 elements on every side: (origin, count, result, count, target, count)
TRIPLES = {
    "indexed-vector1-contig": (IX, 30, V1, 1, F, 420),
    "contig-indexed-subarray2": (F, 420, IX2, 30, SUB2, 14),
    "vector16-subarray3-indexed": (V16, 1, SUB3, 7, IX3, 30),
    "all-three-indexed": (IX, 30, IX2, 30, IX3, 30),
    "subarray2-subarray3-vector16": (SUB2, 14, SUB3, 7, V16, 1),
    "subarray3-contig-vector1": (SUB3, 7, F, 420, V1, 1),
}


# ---- layouts -------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(TRIPLES))
def test_layout_triples(L, name):
    """Regular (one- and two-level) and irregular layouts on every side; every
    side is irregular (a run table and its binary search) at least once, and one
    case on all three."""
    t = TRIPLES[name]
    _run(L, "MPI_SUM", "MPI_FLOAT", *t, 3)
    _run(L, "MPI_REPLACE", None, *t, 3)


@pytest.mark.parametrize("n", [1, W - 1, W, W + 1, 2 * W + 3])
def test_element_counts_around_the_workgroup(L, n):
    o, r, t = ("vector", n, 1, 5, F), ("vector", n, 1, 2, F), ("vector", n, 1, 3, F)
    path = 1 if n == 1 else 3                   # one element is one piece on every side
    _run(L, "MPI_SUM", "MPI_FLOAT", o, 1, r, 1, t, 1, path)
    _run(L, "MPI_REPLACE", None, o, 1, r, 1, t, 1, path)
    _run(L, "MPI_SUM", "MPI_FLOAT", ("indexed", [n], [1], F), 1, IX, (n + 13) // 14, t, 1, path)


def test_origin_smaller_than_the_target_last_instance_partly_covered(L):
    """50 origin elements into two 30-element target instances: the second is
    covered up to its 20th element, the rest of it keeps its values; the result
    has room for 56."""
    o = ("vector", 50, 1, 2, F)
    t = ("resized", 0, 400, ("vector", 30, 1, 3, F))
    first50 = ("hindexed", [1] * 50, [12 * k for k in range(30)] + [400 + 12 * k for k in range(20)], F)
    _run(L, "MPI_SUM", "MPI_FLOAT", o, 1, IX, 4, t, 2, 3, tprefix=(first50, 1))
    _run(L, "MPI_MAX", "MPI_DOUBLE", ("vector", 50, 1, 2, D), 7, ("vector", 60, 1, 3, D), 6, ("vector", 70, 1, 2, D), 5, 3)
    _run(L, "MPI_REPLACE", None, o, 1, IX, 4, t, 2, 3)


def test_result_larger_than_n_keeps_its_tail(L):
    """37 elements; the result triple maps 4 x 37 and the target 2 x 37: the
    mapped elements past n keep their bytes on both sides."""
    o, r, t = ("vector", 37, 1, 5, F), ("vector", 37, 1, 2, F), ("vector", 37, 1, 3, F)
    _run(L, "MPI_SUM", "MPI_FLOAT", o, 1, r, 4, t, 1, 3)
    _run(L, "MPI_SUM", "MPI_FLOAT", o, 1, r, 4, t, 2, 3, tprefix=(t, 1))
    _run(L, "MPI_REPLACE", None, o, 1, r, 4, t, 2, 3)


# ---- the unaligned form ------------------------------------------------------------

@pytest.mark.parametrize("mis", [(1, 0, 0), (0, 1, 0), (0, 0, 1), (3, 2, 1)], ids=lambda m: "o%dr%dt%d" % m)
def test_base_pointers_off_the_element_alignment(L, mis):
    _run(L, "MPI_SUM", "MPI_FLOAT", ("vector", W + 1, 1, 5, F), 1, ("vector", W + 1, 1, 2, F), 1,
         ("vector", W + 1, 1, 3, F), 1, 3, mis)
    m8 = tuple(4 * m for m in mis)
    _run(L, "MPI_SUM", "MPI_DOUBLE", ("vector", 2 * W + 9, 1, 5, D), 1, ("vector", 2 * W + 9, 1, 2, D), 1,
         ("vector", 2 * W + 9, 1, 3, D), 1, 3, m8)
    _run(L, "MPI_REPLACE", None, ("vector", W + 1, 1, 5, F), 1, ("vector", W + 1, 1, 2, F), 1,
         ("vector", W + 1, 1, 3, F), 1, 3, mis)


def test_hindexed_with_odd_byte_displacements(L):
    odd = ("hindexed", [2, 1, 3], [1, 15, 29], F)
    v = ("vector", 6, 1, 2, F)
    _run(L, "MPI_SUM", "MPI_FLOAT", odd, 50, v, 50, v, 50, 3)
    _run(L, "MPI_SUM", "MPI_FLOAT", v, 50, odd, 50, v, 50, 3)
    _run(L, "MPI_PROD", "MPI_FLOAT", v, 50, v, 50, odd, 50, 3)


# ---- the ops -------------------------------------------------------------------------

@pytest.mark.parametrize("pair", [("MPI_SUM", "MPI_FLOAT"), ("MPI_SUM", "MPI_DOUBLE"), ("MPI_SUM", "MPI_INT"),
                                  ("MPI_SUM", "MSX_BFLOAT16"), ("MPI_MAX", "MSX_FLOAT16"), ("MPI_BXOR", "MPI_UINT8_T"),
                                  ("MPI_PROD", "MPI_C_FLOAT_COMPLEX"), ("MPI_MINLOC", "MPI_2INT"),
                                  ("MPI_SUM", "MPI_C_DOUBLE_COMPLEX")],
                         ids=lambda p: f"{p[0]}-{p[1]}")
def test_ops_and_element_sizes(L, pair):
    """2 W + 3 elements through the three-layout kernel with the edge-value
    operands of _cases.gen: element sizes 1, 2, 4, 8 and 16."""
    op, dt = pair
    e = ("basic", h(dt))
    n = 2 * W + 3
    assert _run(L, op, dt, ("vector", n, 1, 2, e), 1, ("vector", n, 1, 4, e), 1, ("vector", n, 1, 3, e), 1, 3)[2] \
        == _esz(dt)


def _mixed(G):
    """A mixed struct whose layout moves in granules of exactly G bytes."""
    i8, i16, i32, i64_, f8 = (("basic", getattr(C, n)) for n in ("MPI_INT8_T", "MPI_INT16_T", "MPI_INT32_T",
                                                                  "MPI_INT64_T", "MPI_DOUBLE"))
    return {1: ("struct", [1, 1], [0, 8], [i8, f8]), 2: ("struct", [1, 1], [0, 8], [i16, f8]),
            4: ("struct", [1, 1], [0, 8], [i32, f8]), 8: ("struct", [1, 2], [0, 16], [i64_, F]),
            16: ("struct", [2, 4], [0, 32], [i64_, F])}[G]


@pytest.mark.parametrize("G", [1, 2, 4, 8, 16])
def test_replace_with_a_mixed_struct_at_each_granule(L, G):
    m = _mixed(G)
    size = build_oracle(m).size
    blocks = 40 * size // G
    tgt = ("vector", blocks, G, 3 * G, ("basic", C.MPI_BYTE))
    assert _run(L, "MPI_REPLACE", None, m, 40, m, 40, tgt, 1, 3)[2] == G
    assert _run(L, "MPI_REPLACE", None, tgt, 1, m, 40, m, 40, 3)[2] == G
    # the pointers count as well: 16-byte granules at a 4-byte offset move in 4-byte granules
    if G == 16:
        _run(L, "MPI_REPLACE", None, m, 40, m, 40, tgt, 1, 3, (4, 8, 0))


def test_no_op_is_a_get_and_takes_no_origin(L):
    """MPI_NO_OP with the origin NULL: the result gets the target's first n
    elements, n counted by the result triple; the target is unchanged."""
    assert _run(L, "MPI_NO_OP", None, None, 0, V1, 1, SUB3, 7, 2)[0] == 420
    _run(L, "MPI_NO_OP", None, None, 0, IX, 30, F, 420, 2)
    _run(L, "MPI_NO_OP", None, None, 0, F, 420, IX2, 30, 2)
    # n ends inside a target instance: 3 x 14 of 60 elements
    _run(L, "MPI_NO_OP", None, None, 0, IX, 3, SUB3, 1, 2)
    # all contiguous: the engine copy
    _run(L, "MPI_NO_OP", None, None, 0, F, 1000, ("contig", 10, F), 100, 1)


# ---- the contiguous path -------------------------------------------------------------

def test_three_contiguous_pieces_are_the_fetch_kernel(L):
    for n in (1, 1000, 4099):
        _run(L, "MPI_SUM", "MPI_FLOAT", F, n, F, n, F, n, 1)
    _run(L, "MPI_SUM", "MPI_FLOAT", ("contig", 10, F), 30, F, 400, ("contig", 3, F), 100, 1)
    _run(L, "MPI_MAXLOC", "MPI_2INT", ("basic", C.MPI_2INT), 300, ("contig", 3, ("basic", C.MPI_2INT)), 100,
         ("basic", C.MPI_2INT), 300, 1)
    _run(L, "MPI_REPLACE", None, F, 1000, ("contig", 10, F), 100, F, 1000, 1)
    # inside the first run of a strided result and target
    _run(L, "MPI_SUM", "MPI_FLOAT", F, 3, ("vector", 5, 4, 6, F), 1, ("vector", 5, 4, 6, F), 1, 1,
         tprefix=(("contig", 3, F), 1))


# ---- overlapping spans, stream order -------------------------------------------------

def test_result_and_target_are_two_columns_of_one_matrix(L):
    """Column j of a 300 x 7 fp32 matrix is the target and column k the result;
    the origin is a column of another matrix.  The spans of result and target
    interleave element by element."""
    rows, cols, j, k = 300, 7, 2, 5
    keep = []
    col = _commit(L, ("vector", rows, 1, cols, F), keep)
    ocol = _commit(L, ("vector", rows, 1, 3, F), keep)
    rng = np.random.default_rng(7)
    m = rng.uniform(-4, 4, (rows, cols)).astype(np.float32)
    src = rng.uniform(-4, 4, (rows, 3)).astype(np.float32)
    exp = m.copy()
    a, b = np.ascontiguousarray(src[:, 1]), np.ascontiguousarray(m[:, j])
    assert oracle.reduce_local(C.MPI_SUM, C.MPI_FLOAT, a, b) == 0
    exp[:, k] = m[:, j]
    exp[:, j] = b
    d = torch.from_numpy(m.copy()).cuda()
    d_src = torch.from_numpy(src.copy()).cuda()
    assert _plan(L, 1, ocol, 1, col, 1, col, C.MPI_SUM) == (rows, 3, 4)
    torch.cuda.synchronize()
    rc = L.msx_get_accumulate_dev(d_src.data_ptr() + 4, 1, ocol, d.data_ptr() + 4 * k, 1, col,
                                  d.data_ptr() + 4 * j, 1, col, C.MPI_SUM, _stream())
    assert rc == 0, msx.last_error()
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy().view(np.uint32), exp.view(np.uint32))
    assert np.array_equal(d_src.cpu().numpy().view(np.uint32), src.view(np.uint32))
    free_all(L, keep)


def test_stream_order(L):
    """On a non-default stream: a copy that writes the origin, the call, and the
    readbacks, all enqueued on that stream with no host synchronisation between
    them; only the stream is synchronised before the check."""
    n = 3 * W + 5
    keep = []
    oh, rh, th = (_commit(L, ("vector", n, 1, s, F), keep) for s in (5, 2, 3))
    rng = np.random.default_rng(11)
    a, b = rng.uniform(-4, 4, (n, 5)).astype(np.float32), rng.uniform(-4, 4, (n, 3)).astype(np.float32)
    r0 = rng.uniform(-4, 4, (n, 2)).astype(np.float32)
    exp_t, exp_r = b.copy(), r0.copy()
    col = np.ascontiguousarray(b[:, 0])
    assert oracle.reduce_local(C.MPI_SUM, C.MPI_FLOAT, np.ascontiguousarray(a[:, 0]), col) == 0
    exp_t[:, 0] = col
    exp_r[:, 0] = b[:, 0]
    d_o = torch.zeros(n, 5, dtype=torch.float32, device="cuda")            # not the origin yet
    d_t, d_r = torch.from_numpy(b.copy()).cuda(), torch.from_numpy(r0.copy()).cuda()
    src = torch.from_numpy(a.copy()).pin_memory()
    back_t = torch.empty(n, 3, dtype=torch.float32).pin_memory()
    back_r = torch.empty(n, 2, dtype=torch.float32).pin_memory()
    assert _plan(L, 1, oh, 1, rh, 1, th, C.MPI_SUM) == (n, 3, 4)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_o.copy_(src, non_blocking=True)
        rc = L.msx_get_accumulate_dev(d_o.data_ptr(), 1, oh, d_r.data_ptr(), 1, rh, d_t.data_ptr(), 1, th, C.MPI_SUM,
                                      ctypes.c_void_p(s.cuda_stream))
        back_t.copy_(d_t, non_blocking=True)
        back_r.copy_(d_r, non_blocking=True)
    assert rc == 0, msx.last_error()
    s.synchronize()
    assert np.array_equal(back_t.numpy().view(np.uint32), exp_t.view(np.uint32))
    assert np.array_equal(back_r.numpy().view(np.uint32), exp_r.view(np.uint32))
    free_all(L, keep)


# ---- 2^32 elements and more: the 64-bit address map ----------------------------------

@pytest.mark.parametrize("op", ["MPI_SUM", "MPI_REPLACE"])
def test_more_than_4_gi_elements(L, op):
    """2049 instances of two 1 MiB rows of int8, 2^32 + 2^21 elements: the
    element index no longer fits the 32-bit divisions, so every workgroup runs
    the serial form.  Rows of 1 MiB + 16 bytes (origin) into rows of 1 MiB + 48
    (target), the old rows out to rows of 1 MiB + 32 (result); torch computes
    the reference on the GPU.  MPI_REPLACE runs from an origin one byte off
    alignment, so it moves single bytes and its granule index passes 2^32 too."""
    row, po, pr, pt, inst = 1 << 20, 16, 32, 48, 2049
    i8 = ("basic", C.MPI_INT8_T)
    keep = []
    oh, rh, th = (_commit(L, ("resized", 0, 2 * (row + p), ("vector", 2, row, row + p, i8)), keep) for p in (po, pr, pt))
    mis = 1 if op == "MPI_REPLACE" else 0
    g = torch.Generator(device="cuda").manual_seed(5)
    d_o = torch.randint(-128, 128, (2 * inst * (row + po) + 16,), dtype=torch.int8, device="cuda", generator=g)
    d_t = torch.randint(-128, 128, (2 * inst, row + pt), dtype=torch.int8, device="cuda", generator=g)
    d_r = torch.randint(-128, 128, (2 * inst, row + pr), dtype=torch.int8, device="cuda", generator=g)
    ov = d_o[mis:mis + 2 * inst * (row + po)].view(2 * inst, row + po)
    o_before = d_o.clone()
    exp_t, exp_r = d_t.clone(), d_r.clone()
    exp_r[:, :row] = d_t[:, :row]
    exp_t[:, :row] = ov[:, :row] if op == "MPI_REPLACE" else exp_t[:, :row] + ov[:, :row]      # int8 wraps
    n, path, gran = _plan(L, inst, oh, inst, rh, inst, th, h(op))
    assert (n, path) == (2 * inst * row, 3) and n > 1 << 32
    torch.cuda.synchronize()
    rc = L.msx_get_accumulate_dev(d_o.data_ptr() + mis, inst, oh, d_r.data_ptr(), inst, rh, d_t.data_ptr(), inst, th,
                                  h(op), _stream())
    assert rc == 0, msx.last_error()
    torch.cuda.synchronize()
    assert torch.equal(d_t, exp_t)
    assert torch.equal(d_r, exp_r)
    assert torch.equal(d_o, o_before)
    free_all(L, keep)
