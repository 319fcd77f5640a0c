"""GPU: msx_accumulate_batch_dev (the multi-segment two-layout kernels of
msx_acc2_segs.hip) against an independent numpy reference, byte for byte.

A case is a list of origin arenas, a list of target arenas and a list of
segments, each naming an arena and a buffer address inside it on either side;
several segments' targets may be carved from ONE arena, so that their spans
interleave.  Arenas are sentinel-filled with 64 guard bytes at either end.  The
reference takes the type maps from oracle/msx_dtype_oracle.py (element by
element), gathers and combines with the oracle's op.cpp restatement
(_half_ref.combine for the 16-bit floats) and scatters.  After every call
  * every target arena equals its expected image, so every unmapped byte kept
    its value;
  * every origin arena is unchanged;
  * the target arenas equal the ones the same inputs give through
    msx_accumulate_dev segment by segment -- the definition of the call.
The plan (msx_accumulate_batch_plan) is asserted before each call, so each case
is known to be fused as meant."""
import ctypes
import zlib

import numpy as np
import pytest

import msx
import oracle
from _cases import h
from test_dtype_cpu import build_oracle, free_all
from test_gpu_accumulate_dev import (F, GUARD, IX, IX2, PAT_O, PAT_T, W, L, _arena, _commit, _data_bytes,  # noqa: F401
                                     _pairs, _same, _stream, _up)
from test_gpu_batch_local import _data, _esz, _ref

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

C = msx.C
vp, i64, c_int = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
EMPTY = None                 # an empty segment: null pointers, zero counts


class Seg:
    """Origin triple (arena oa, buffer address ob inside it) into a target triple."""
    def __init__(self, oa, ob, orec, ocount, ta, tb, trec, tcount):
        self.oa, self.ob, self.orec, self.ocount = oa, ob, orec, ocount
        self.ta, self.tb, self.trec, self.tcount = ta, tb, trec, tcount


@pytest.fixture(scope="module")
def limits(L):
    return _plan(L, [], [], C.MPI_SUM)[:2]


def _arr(ct, vals):
    return (ct * max(len(vals), 1))(*vals)


def _plan(L, segs, handles, op):
    """(width, fuse_below, launches, batched, single)"""
    oc = _arr(i64, [0 if s is EMPTY else s.ocount for s in segs])
    tc = _arr(i64, [0 if s is EMPTY else s.tcount for s in segs])
    od, td = _arr(c_int, [x[0] for x in handles]), _arr(c_int, [x[1] for x in handles])
    w, fb, la, ba, si = c_int(-7), i64(-7), c_int(-7), c_int(-7), c_int(-7)
    rc = L.msx_accumulate_batch_plan(oc, od, tc, td, len(segs), op, ctypes.byref(w), ctypes.byref(fb), ctypes.byref(la),
                                     ctypes.byref(ba), ctypes.byref(si))
    assert rc == 0, msx.last_error()
    return w.value, fb.value, la.value, ba.value, si.value


def _single_path(L, s, hd, op):
    n, path, gran = i64(), c_int(), c_int()
    assert L.msx_accumulate_plan(s.ocount, hd[0], s.tcount, hd[1], op, ctypes.byref(n), ctypes.byref(path),
                                 ctypes.byref(gran)) == 0, msx.last_error()
    return path.value


def _simple(op, dt, specs, seed=0):
    """One origin arena and one target arena per segment.  specs: EMPTY or
    (origin recipe, count, target recipe, count[, mis_o, mis_t]); dt None fills
    random bytes (MPI_REPLACE / MPI_NO_OP)."""
    rng = np.random.default_rng(zlib.crc32(f"acc2batch/{op}/{dt}/{seed}/{len(specs)}".encode()))
    o_imgs, t_imgs, segs = [], [], []
    for sp in specs:
        if sp is EMPTY:
            segs.append(EMPTY)
            continue
        orec, ocount, trec, tcount = sp[:4]
        mis_o, mis_t = sp[4:6] if len(sp) > 4 else (0, 0)
        ot, tt = build_oracle(orec), build_oracle(trec)
        img_o, bo = _arena(ot, ocount, mis_o, PAT_O)
        img_t, bt = _arena(tt, tcount, mis_t, PAT_T)
        ob, tb = _data_bytes(ot, ocount, bo), _data_bytes(tt, tcount, bt)
        assert ob.size <= tb.size and np.unique(tb).size == tb.size          # a legal target map
        if dt is None:
            img_o[ob] = rng.integers(0, 256, ob.size, dtype=np.uint8)
            img_t[tb] = rng.integers(0, 256, tb.size, dtype=np.uint8)
        else:
            esz = _esz(dt)
            img_o[ob] = _data(op, dt, ob.size // esz, rng)
            img_t[tb] = _data(op, dt, tb.size // esz, rng)
        segs.append(Seg(len(o_imgs), bo, orec, ocount, len(t_imgs), bt, trec, tcount))
        o_imgs.append(img_o)
        t_imgs.append(img_t)
    return o_imgs, t_imgs, segs


def _run(L, op, dt, case, expect, stream=None, paths=None):
    """One msx_accumulate_batch_dev call checked as the module docstring says.
    expect: (launches, batched, single).  paths: the msx_accumulate_plan paths
    the fused segments must show between them.  Returns the target arenas."""
    o_imgs, t_imgs, segs = case
    keep, cache = [], {}

    def handle(rec):
        if repr(rec) not in cache:
            cache[repr(rec)] = _commit(L, rec, keep)
        return cache[repr(rec)]

    handles = [(C.MPI_FLOAT, C.MPI_FLOAT) if s is EMPTY else (handle(s.orec), handle(s.trec)) for s in segs]
    exp = [img.copy() for img in t_imgs]
    for s in segs:
        if s is EMPTY:
            continue
        io = _data_bytes(build_oracle(s.orec), s.ocount, s.ob)
        it = _data_bytes(build_oracle(s.trec), s.tcount, s.tb)[:io.size]
        if op == "MPI_REPLACE":
            exp[s.ta][it] = o_imgs[s.oa][io]
        elif op != "MPI_NO_OP":
            exp[s.ta][it] = _ref(op, dt, o_imgs[s.oa][io], t_imgs[s.ta][it])
    plan = _plan(L, segs, handles, h(op))
    assert plan[2:] == tuple(expect), (plan, expect)
    assert plan[2] == -(-plan[3] // plan[0]) + plan[4]
    if paths is not None:
        assert {_single_path(L, s, hd, h(op)) for s, hd in zip(segs, handles) if s is not EMPTY} == set(paths)

    def addresses(d_o, d_t):
        return (_arr(vp, [None if s is EMPTY else d_o[s.oa].data_ptr() + s.ob for s in segs]),
                _arr(vp, [None if s is EMPTY else d_t[s.ta].data_ptr() + s.tb for s in segs]))

    oc = _arr(i64, [0 if s is EMPTY else s.ocount for s in segs])
    tc = _arr(i64, [0 if s is EMPTY else s.tcount for s in segs])
    od, td = _arr(c_int, [x[0] for x in handles]), _arr(c_int, [x[1] for x in handles])
    d_o, d_t = [_up(i) for i in o_imgs], [_up(i) for i in t_imgs]
    po, pt = addresses(d_o, d_t)
    torch.cuda.synchronize()
    rc = L.msx_accumulate_batch_dev(po, oc, od, pt, tc, td, len(segs), h(op), stream or _stream())
    assert rc == 0, msx.last_error()
    # the host arrays are read during the call only
    for a in (po, pt, oc, tc, od, td):
        ctypes.memset(a, 0xEE, ctypes.sizeof(a))
    torch.cuda.synchronize()
    got = [d.cpu().numpy() for d in d_t]
    for j, (g, e) in enumerate(zip(got, exp)):
        _same(g, e, f"{op} {dt} target arena {j}")
    for j, (d, img) in enumerate(zip(d_o, o_imgs)):
        assert np.array_equal(d.cpu().numpy(), img), f"{op} {dt}: origin arena {j} changed"
    # the definition: msx_accumulate_dev segment by segment on copies of the same arenas
    d_o, d_t = [_up(i) for i in o_imgs], [_up(i) for i in t_imgs]
    torch.cuda.synchronize()
    for s, hd in zip(segs, handles):
        if s is EMPTY:
            continue
        rc = L.msx_accumulate_dev(d_o[s.oa].data_ptr() + s.ob, s.ocount, hd[0], d_t[s.ta].data_ptr() + s.tb, s.tcount,
                                  hd[1], h(op), _stream())
        assert rc == 0, msx.last_error()
    torch.cuda.synchronize()
    for j, (g, d) in enumerate(zip(got, d_t)):
        _same(g, d.cpu().numpy(), f"{op} {dt} target arena {j} vs msx_accumulate_dev")
    free_all(L, keep)
    return got


def _vv(n, e=F, so=5, st=3):
    return ("vector", n, 1, so, e), 1, ("vector", n, 1, st, e), 1


# ---- tile and segment edges ----------------------------------------------------------

@pytest.mark.parametrize("op", ["MPI_SUM", "MPI_REPLACE"])
def test_tile_and_segment_edges_in_one_launch(L, op):
    """1, 255, 256, 257, 513 and 768 elements: the tile -> segment search, whole
    tiles and cut last tiles; empty segments with null pointers in between."""
    specs = [EMPTY, _vv(1), _vv(W - 1), EMPTY, EMPTY, _vv(W), _vv(W + 1), _vv(2 * W + 1), EMPTY, _vv(3 * W), EMPTY]
    dt = "MPI_FLOAT" if op == "MPI_SUM" else None
    _run(L, op, dt, _simple(op, dt, specs), (1, 6, 0), paths={1, 4})    # one element lies inside the first run
    _run(L, op, dt, _simple(op, dt, specs[::-1], seed=1), (1, 6, 0))


def test_only_empty_segments(L):
    _run(L, "MPI_SUM", "MPI_FLOAT", ([], [], [EMPTY, EMPTY, EMPTY]), (0, 0, 0))


# ---- width edges ---------------------------------------------------------------------

@pytest.mark.parametrize("which", ["1", "width", "width+1", "2*width+3"])
def test_width_edges(L, limits, which):
    width = limits[0]
    n = {"1": 1, "width": width, "width+1": width + 1, "2*width+3": 2 * width + 3}[which]
    specs = [_vv(1 + (97 * i) % 300) for i in range(n)]
    _run(L, "MPI_SUM", "MPI_FLOAT", _simple("MPI_SUM", "MPI_FLOAT", specs), (-(-n // width), n, 0))


# ---- regular and irregular sides, every path of the single call ---------------------------

SUB_O = ("subarray", [6, 7, 8], [3, 4, 5], [2, 1, 3], True, F)          # 60 elements, two levels
SUB_T = ("subarray", [7, 9, 4], [5, 6, 2], [1, 3, 1], False, F)
MIXED_SIDES = [
    (("vector", 37, 1, 5, F), 8, SUB_T, 5),                     # one level -> two levels, 296 into 300
    (SUB_O, 5, IX, 25),                                         # two levels -> irregular, 300 into 350
    (IX, 20, ("vector", 14, 1, 2, F), 20),                      # irregular -> one level
    (IX, 20, IX2, 20),                                          # irregular on both sides
    (F, 1000, F, 1000),                                         # predefined handles: path 1
    (("contig", 10, F), 30, F, 400),                            # path 1
    (F, 3, ("vector", 5, 4, 6, F), 1),                          # path 1: inside the target's first run
    (F, 111, ("vector", 37, 1, 3, F), 3),                       # path 2
    (("contig", 14, F), 20, IX, 25),                            # path 2 into an irregular target
    (("vector", 37, 1, 5, F), 9, F, 333),                       # path 3 under MPI_REPLACE, 4 under an op
    (IX, 20, ("contig", 7, F), 50),                             # the same from an irregular origin
    (("contig", 10, F), 4, ("vector", 60, 1, 2, F), 1),         # contiguous into part of an instance: path 4
]


@pytest.mark.parametrize("op", ["MPI_SUM", "MPI_MAX", "MPI_REPLACE"])
def test_regular_irregular_and_contiguous_sides_in_one_launch(L, limits, op):
    assert len(MIXED_SIDES) <= limits[0]
    dt = None if op == "MPI_REPLACE" else "MPI_FLOAT"
    paths = {1, 2, 3, 4} if op == "MPI_REPLACE" else {1, 2, 4}
    _run(L, op, dt, _simple(op, dt, MIXED_SIDES), (1, len(MIXED_SIDES), 0), paths=paths)


def test_unequal_counts_and_negative_strides(L):
    o = ("resized", 0, 100, ("vector", 10, 1, 2, F))
    t = ("resized", 0, 200, ("vector", 15, 1, 3, F))
    neg = ("resized", -16, 136, ("hvector", 10, 1, -12, F))
    specs = [(o, 6, t, 4), (neg, 6, t, 4), (o, 6, ("resized", -16, 208, ("hvector", 15, 1, -12, F)), 4),
             (("vector", 50, 1, 2, F), 1, ("vector", 60, 1, 3, F), 1)]          # a partly covered target instance
    _run(L, "MPI_SUM", "MPI_FLOAT", _simple("MPI_SUM", "MPI_FLOAT", specs), (1, 4, 0))


# ---- alignment -----------------------------------------------------------------------

@pytest.mark.parametrize("dt", ["MPI_INT8_T", "MPI_INT16_T", "MPI_FLOAT", "MPI_DOUBLE", "MPI_C_DOUBLE_COMPLEX"])
@pytest.mark.parametrize("side", ["origin", "target"])
def test_one_misaligned_pointer_among_aligned_segments(L, dt, side):
    """The whole launch runs the unaligned form; every element size."""
    e = ("basic", h(dt))
    mis = max(1, _esz(dt) // 2)
    bad = _vv(W + 1, e) + ((mis, 0) if side == "origin" else (0, mis))
    specs = [_vv(W + 3, e), _vv(40, e), bad, (e, 300, e, 300), _vv(2 * W, e)]
    _run(L, "MPI_SUM", dt, _simple("MPI_SUM", dt, specs), (1, 5, 0))
    _run(L, "MPI_SUM", dt, _simple("MPI_SUM", dt, specs[:2] + specs[3:], seed=1), (1, 4, 0))     # all aligned


def test_odd_byte_displacements_in_one_segment(L):
    odd = ("hindexed", [2, 1, 3], [1, 15, 29], F)
    specs = [_vv(W + 1), (odd, 50, ("vector", 6, 1, 2, F), 50), (("vector", 6, 1, 2, F), 50, odd, 50)]
    _run(L, "MPI_PROD", "MPI_FLOAT", _simple("MPI_PROD", "MPI_FLOAT", specs), (1, 3, 0))


def test_replace_with_granules_16_4_and_1_in_one_call(L):
    b = ("basic", C.MPI_BYTE)
    bv = lambda G: (("vector", 37, G, 3 * G, b), 9, ("vector", 37, G, 5 * G, b), 9)
    for specs in ([bv(16), bv(4), bv(1)], [bv(16), bv(16)], [bv(16), bv(16) + (4, 8)], [bv(8), bv(2), bv(16)]):
        _run(L, "MPI_REPLACE", None, _simple("MPI_REPLACE", None, specs), (1, len(specs), 0))


# ---- the halo --------------------------------------------------------------------------

SHAPE = (20, 24, 28)


def _faces():
    """Six disjoint one-cell faces of a SHAPE array: x whole, y without the x
    edges, z without both: (subsizes, starts)."""
    nx, ny, nz = SHAPE
    return [((1, ny, nz), (0, 0, 0)), ((1, ny, nz), (nx - 1, 0, 0)),
            ((nx - 2, 1, nz), (1, 0, 0)), ((nx - 2, 1, nz), (1, ny - 1, 0)),
            ((nx - 2, ny - 2, 1), (1, 1, 0)), ((nx - 2, ny - 2, 1), (1, 1, nz - 1))]


@pytest.mark.parametrize("origin", ["buffers", "faces"])
def test_halo_sum_of_six_faces_is_one_launch(L, origin):
    """All six targets are one array (one address, six datatype handles); the
    origins are six contiguous receive buffers, or the faces of a second array."""
    rng = np.random.default_rng(20 if origin == "buffers" else 21)
    n = int(np.prod(SHAPE))
    arr = rng.uniform(-4, 4, SHAPE).astype(np.float32)
    img_t = np.full(n * 4 + 2 * GUARD, PAT_T, np.uint8)
    img_t[GUARD:GUARD + 4 * n] = np.frombuffer(arr.tobytes(), np.uint8)
    o_imgs, segs = [], []
    if origin == "faces":
        img_o = np.full(n * 4 + 2 * GUARD, PAT_O, np.uint8)
        img_o[GUARD:GUARD + 4 * n] = np.frombuffer(rng.uniform(-4, 4, SHAPE).astype(np.float32).tobytes(), np.uint8)
        o_imgs.append(img_o)
    for sub, start in _faces():
        face = ("subarray", list(SHAPE), list(sub), list(start), True, F)
        m = int(np.prod(sub))
        if origin == "buffers":
            img_o = np.full(m * 4 + 2 * GUARD, PAT_O, np.uint8)
            img_o[GUARD:GUARD + 4 * m] = np.frombuffer(rng.uniform(-4, 4, m).astype(np.float32).tobytes(), np.uint8)
            segs.append(Seg(len(o_imgs), GUARD, F, m, 0, GUARD, face, 1))
            o_imgs.append(img_o)
        else:
            segs.append(Seg(0, GUARD, face, 1, 0, GUARD, face, 1))
    got = _run(L, "MPI_SUM", "MPI_FLOAT", (o_imgs, [img_t], segs), (1, 6, 0))
    # every non-face cell of the array is unchanged, every face cell was written once
    out = np.frombuffer(got[0][GUARD:GUARD + 4 * n].tobytes(), np.float32).reshape(SHAPE)
    inner = (slice(1, -1),) * 3
    assert np.array_equal(out[inner].view(np.uint32), arr[inner].view(np.uint32))
    touched = np.zeros(SHAPE, np.int32)
    for sub, start in _faces():
        touched[tuple(slice(a, a + b) for a, b in zip(start, sub))] += 1
    assert touched.max() == 1 and np.array_equal(touched == 0, np.pad(np.ones(tuple(x - 2 for x in SHAPE), bool), 1))


# ---- every (op, element kind) pair -------------------------------------------------------

@pytest.mark.parametrize("pair", _pairs(), ids=lambda p: f"{p[0]}-{p[1]}")
def test_every_op_and_element_kind(L, pair):
    """Three small segments per pair: a cut tile through the two-layout map, a
    contiguous pair of predefined handles and an irregular origin."""
    op, dt = pair
    e = ("basic", h(dt))
    ix = ("indexed", [3, 1, 4, 1, 5], [0, 5, 7, 13, 16], e)
    specs = [_vv(W + 1, e, 2, 3), (e, 7, e, 7), (ix, 3, ("vector", 42, 1, 2, e), 1)]
    _run(L, op, dt, _simple(op, dt, specs), (1, 3, 0))


def test_replace_on_a_mixed_struct(L):
    i8, f8 = ("basic", C.MPI_INT8_T), ("basic", C.MPI_DOUBLE)
    o = ("struct", [1, 1], [0, 8], [i8, f8])
    t = ("struct", [1, 1], [16, 0], [i8, f8])
    specs = [(o, 40, t, 40), (o, 40, ("vector", 90, 1, 2, F), 1), _vv(W + 1, ("basic", C.MPI_INT)), _vv(70)]
    _run(L, "MPI_REPLACE", None, _simple("MPI_REPLACE", None, specs), (1, 4, 0))


def test_no_op_writes_nothing(L):
    specs = [_vv(37), (("struct", [1, 1], [0, 8], [("basic", C.MPI_INT8_T), ("basic", C.MPI_DOUBLE)]), 3, F, 9)]
    _run(L, "MPI_NO_OP", None, _simple("MPI_NO_OP", None, specs), (0, 0, 0))


# ---- the fuse limit ------------------------------------------------------------------------

def test_a_segment_at_the_fuse_limit_between_two_small_ones(L, limits):
    n = limits[1] // 4
    specs = [_vv(W + 1), (F, n, F, n), _vv(3 * W + 5)]
    _run(L, "MPI_SUM", "MPI_FLOAT", _simple("MPI_SUM", "MPI_FLOAT", specs), (2, 2, 1))


# ---- stream ordering -------------------------------------------------------------------------

def test_stream_order(L):
    """On a non-default stream: a copy that writes the origins, the call, and the
    readback, all enqueued on that stream with no host synchronisation between
    them; only the stream is synchronised before the check."""
    counts = (3 * W + 5, W, 41)
    keep = []
    rng = np.random.default_rng(13)
    total = sum(counts)
    a, b = rng.uniform(-4, 4, (total, 5)).astype(np.float32), rng.uniform(-4, 4, (total, 3)).astype(np.float32)
    exp = b.copy()
    col = np.ascontiguousarray(b[:, 0])
    assert oracle.reduce_local(C.MPI_SUM, C.MPI_FLOAT, np.ascontiguousarray(a[:, 0]), col) == 0
    exp[:, 0] = col
    d_o = torch.zeros(total, 5, dtype=torch.float32, device="cuda")           # not the origins yet
    d_t = torch.from_numpy(b.copy()).cuda()
    src = torch.from_numpy(a.copy()).pin_memory()
    back = torch.empty(total, 3, dtype=torch.float32).pin_memory()
    po, pt, od, td, row = [], [], [], [], 0
    for n in counts:                                                          # column 0 of three row blocks
        od.append(_commit(L, ("vector", n, 1, 5, F), keep))
        td.append(_commit(L, ("vector", n, 1, 3, F), keep))
        po.append(d_o.data_ptr() + 20 * row)
        pt.append(d_t.data_ptr() + 12 * row)
        row += n
    one = _arr(i64, [1, 1, 1])
    w, fb, la, ba, si = c_int(), i64(), c_int(), c_int(), c_int()
    assert L.msx_accumulate_batch_plan(one, _arr(c_int, od), one, _arr(c_int, td), 3, C.MPI_SUM, ctypes.byref(w),
                                       ctypes.byref(fb), ctypes.byref(la), ctypes.byref(ba), ctypes.byref(si)) == 0
    assert (la.value, ba.value, si.value) == (1, 3, 0)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_o.copy_(src, non_blocking=True)
        rc = L.msx_accumulate_batch_dev(_arr(vp, po), one, _arr(c_int, od), _arr(vp, pt), one, _arr(c_int, td), 3,
                                        C.MPI_SUM, ctypes.c_void_p(s.cuda_stream))
        back.copy_(d_t, non_blocking=True)
    assert rc == 0, msx.last_error()
    s.synchronize()
    assert np.array_equal(back.numpy().view(np.uint32), exp.view(np.uint32))
    free_all(L, keep)
