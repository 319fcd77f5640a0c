"""GPU: msx_reduce_local_batch_dev (k_combine_segs, many small combines in one
launch) against the oracle, bit for bit.

Segments are carved out of one device arena per operand with 64 guard bytes of
a fixed pattern between them.  After every call three things must hold:
  * every segment's bytes equal the reference's (the oracle; _half_ref.combine
    for the 16-bit floats);
  * every guard byte of the inout arena and the whole `in` arena are unchanged;
  * the inout arena equals the one the same inputs give through
    msx_reduce_local_dev segment by segment -- the definition of the call.
The plan (msx_reduce_local_batch_plan) of every batch is checked against the
rule in include/msx.h, which shows that the segments really were fused."""
import ctypes
import zlib

import numpy as np
import pytest

import msx
import oracle
import _half_ref as R
from _cases import KIND, gen, h, itemsize, legal_pairs, np_dtype

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

C = msx.C
vp, i64 = ctypes.c_void_p, ctypes.c_int64
GUARD = 64
PAT_IN, PAT_IO = 0x5A, 0xA5
LIMIT = 16 << 20           # bytes per operand from which a segment is launched on its own (msx.h)
SCALAR_MAX = 64 << 10      # the same for operands at different offsets from 16-byte alignment


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    lib = msx.init(errors_return=True)
    assert lib.msx_device_count() > 0
    return lib


@pytest.fixture(scope="module")
def width(L):
    out = [ctypes.c_int() for _ in range(4)]
    assert L.msx_reduce_local_batch_plan(None, None, None, 0, C.MPI_FLOAT, C.MPI_SUM,
                                         *[ctypes.byref(o) for o in out]) == 0
    assert out[0].value >= 16
    return out[0].value


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _esz(dt):
    return 2 if dt in R.TYPES else itemsize(KIND[dt])


def _data(op, dt, n, rng):
    """n elements of `dt` as bytes, edge values mixed in."""
    if dt in R.TYPES:
        x = rng.integers(0, 1 << 16, n, dtype=np.uint32).astype(np.uint16)
        sel = rng.random(n) < 0.25
        x[sel] = R.partners(dt)[rng.integers(0, 64, int(sel.sum()))]
        return np.frombuffer(x.tobytes(), np.uint8)
    return np.frombuffer(gen(KIND[dt], op, n, rng).tobytes(), np.uint8)


def _ref(op, dt, a, b):
    """Bytes of `b (op)= a` by the reference."""
    if a.size == 0:
        return b
    if dt in R.TYPES:
        o = "MPI_SUM" if op == "MSX_SUM_WIDE" else op
        r = R.combine(o, dt, np.frombuffer(b.tobytes(), np.uint16), np.frombuffer(a.tobytes(), np.uint16))
        return np.frombuffer(r.tobytes(), np.uint8)
    t = np_dtype(KIND[dt])
    x = np.frombuffer(bytearray(a.tobytes()), t)
    exp = np.frombuffer(bytearray(b.tobytes()), t)
    assert oracle.reduce_local(h(op), h(dt), x, exp) == 0
    return np.frombuffer(exp.tobytes(), np.uint8)


def _layout(segs):
    """segs: (in bytes, inout bytes, off_in, off_io), the offsets from 16-byte
    alignment.  Returns the two arena images and the segments' positions."""
    up16 = lambda v: (v + 15) // 16 * 16
    pin, pio, ci, co = [], [], GUARD, GUARD
    for a, b, oi, oo in segs:
        assert a.size == b.size
        pin.append(ci + oi)
        pio.append(co + oo)
        ci = up16(ci + oi + a.size + GUARD)
        co = up16(co + oo + b.size + GUARD)
    img_in, img_io = np.full(ci, PAT_IN, np.uint8), np.full(co, PAT_IO, np.uint8)
    for (a, b, _, _), pi, po in zip(segs, pin, pio):
        img_in[pi:pi + a.size] = a
        img_io[po:po + b.size] = b
    return img_in, img_io, pin, pio


def _up(img):
    t = torch.from_numpy(img.copy()).pin_memory().cuda()
    assert t.data_ptr() % 16 == 0
    return t


def _expected(op, dt, segs, img_io, pio):
    exp = img_io.copy()
    for (a, b, _, _), po in zip(segs, pio):
        exp[po:po + b.size] = _ref(op, dt, a, b)
    return exp


def _same(got, exp, segs, pio, tag):
    if np.array_equal(got, exp):
        return
    i = int(np.nonzero(got != exp)[0][0])
    where = "a guard byte"
    for k, ((a, _, _, _), po) in enumerate(zip(segs, pio)):
        if po <= i < po + a.size:
            where = f"segment {k} ({a.size} bytes) byte {i - po}"
    pytest.fail(f"{tag}: {int((got != exp).sum())} bytes differ, first in {where}: "
                f"got {int(got[i]):#04x} exp {int(exp[i]):#04x}")


def _want_plan(dt, segs, pin, pio, width):
    batched = single = 0
    for (a, _, _, _), pi, po in zip(segs, pin, pio):
        if a.size == 0:
            continue
        apart = pi % 16 != po % 16
        if a.size >= LIMIT or (apart and a.size >= SCALAR_MAX):
            single += 1
        else:
            batched += 1
    return -(-batched // width) + single, batched, single


def _run(L, width, op, dt, segs, null_empty=()):
    """One batch call over `segs`, checked as the module docstring says.
    null_empty: indices of empty segments that get null pointers."""
    esz = _esz(dt)
    n = len(segs)
    img_in, img_io, pin, pio = _layout(segs)
    t_in, t_io, t_one = _up(img_in), _up(img_io), _up(img_io)
    counts = [a.size // esz for a, _, _, _ in segs]
    for k in null_empty:
        assert counts[k] == 0
    pa = [None if k in null_empty else t_in.data_ptr() + p for k, p in enumerate(pin)]
    pb = [None if k in null_empty else t_io.data_ptr() + p for k, p in enumerate(pio)]
    A, B, N = (vp * n)(*pa), (vp * n)(*pb), (i64 * n)(*counts)
    out = [ctypes.c_int(-1) for _ in range(4)]
    assert L.msx_reduce_local_batch_plan(A, B, N, n, h(dt), h(op), *[ctypes.byref(o) for o in out]) == 0, \
        msx.last_error()
    plan = tuple(o.value for o in out)
    assert plan == (width,) + _want_plan(dt, segs, pin, pio, width), (op, dt)
    torch.cuda.synchronize()      # the uploads went through torch's stream machinery
    rc = L.msx_reduce_local_batch_dev(A, B, N, n, h(dt), h(op), _stream())
    assert rc == 0, msx.last_error()
    torch.cuda.synchronize()
    got = t_io.cpu().numpy()
    _same(got, _expected(op, dt, segs, img_io, pio), segs, pio, f"{op} {dt} batch of {n}")
    assert np.array_equal(t_in.cpu().numpy(), img_in), f"{op} {dt}: the `in` arena changed"
    # the definition: msx_reduce_local_dev segment by segment
    for k in range(n):
        if counts[k]:
            rc = L.msx_reduce_local_dev(t_in.data_ptr() + pin[k], t_one.data_ptr() + pio[k], counts[k], h(dt),
                                        h(op if op != "MSX_SUM_WIDE" else "MPI_SUM"), _stream())
            assert rc == 0, msx.last_error()
    torch.cuda.synchronize()
    _same(got, t_one.cpu().numpy(), segs, pio, f"{op} {dt} batch vs msx_reduce_local_dev")
    return plan


def _seg(op, dt, count, rng, off_in=0, off_io=0):
    return _data(op, dt, count, rng), _data(op, dt, count, rng), off_in, off_io


_HALF_PAIRS = [(op, dt) for dt in R.TYPES for op in R.OPS]


@pytest.mark.parametrize("pair", legal_pairs(oracle) + _HALF_PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_every_legal_pair_at_the_vector_and_tile_boundaries(L, width, pair):
    """One batch per (op, datatype): element counts around the 16-byte vector
    (EPV elements), the 256-vector tile and a third tile with head and tail,
    each at a common offset of 0, one element and 16 bytes minus one element
    (16-byte types: also their natural 8, where every element runs as a
    scalar)."""
    op, dt = pair
    esz = _esz(dt)
    epv = 16 // esz
    rng = np.random.default_rng(zlib.crc32(f"batch/{op}/{dt}".encode()))
    offs = sorted({0, esz % 16, (16 - esz) % 16} | ({8} if esz == 16 else set()))
    segs = []
    for n in (0, 1, epv - 1, epv, epv + 1, 256 * epv - 1, 256 * epv, 256 * epv + 1, 2 * 256 * epv + epv + 1):
        for off in offs:
            segs.append(_seg(op, dt, n, rng, off, off))
    plan = _run(L, width, op, dt, segs)
    assert plan[3] == 0 and plan[1] == -(-plan[2] // width)       # every segment fused


@pytest.mark.parametrize("dt", ["MPI_FLOAT", "MPI_INT8_T", "MPI_SHORT", "MPI_DOUBLE", "MPI_DOUBLE_INT",
                                "MPI_C_DOUBLE_COMPLEX", "MPI_SHORT_INT", "MSX_BFLOAT16"])
def test_mutually_misaligned_segments(L, width, dt):
    """`in` and `inout` at different offsets from 16-byte alignment, mixed with
    aligned segments: 5 and 4099 elements, and one element either side of the
    64 KiB at which such a segment leaves the fused launch for the realigning
    kernel."""
    esz = _esz(dt)
    op = "MPI_MAXLOC" if dt not in R.TYPES and KIND[dt] in msx.LOC_DTYPES else "MPI_SUM"
    off = esz if esz < 16 else 8
    rng = np.random.default_rng(zlib.crc32(f"apart/{dt}".encode()))
    segs = []
    for n in (5, 4099, SCALAR_MAX // esz - 1, SCALAR_MAX // esz):
        segs.append(_seg(op, dt, n, rng, off, 0))
        segs.append(_seg(op, dt, 300, rng))
        segs.append(_seg(op, dt, n, rng, 0, off))
        segs.append(_seg(op, dt, 7, rng, off, off))
    plan = _run(L, width, op, dt, segs)
    assert plan[3] >= 2 and plan[2] >= 12          # both kinds in one call


@pytest.mark.parametrize("shape", ["1", "2", "w-1", "w", "w+1", "2w+1"])
def test_segment_lookup(L, width, shape):
    """Segment counts around the fused launch's width, 3 to 700 fp32 elements
    each, with empty segments first, last and in runs in the middle (some with
    null pointers)."""
    nseg = {"1": 1, "2": 2, "w-1": width - 1, "w": width, "w+1": width + 1, "2w+1": 2 * width + 1}[shape]
    rng = np.random.default_rng(zlib.crc32(f"lookup/{shape}".encode()))
    segs, null_empty = [], []
    empty = lambda: segs.append(_seg("MPI_SUM", "MPI_FLOAT", 0, rng))
    empty()
    null_empty.append(0)
    for k in range(nseg):
        segs.append(_seg("MPI_SUM", "MPI_FLOAT", int(rng.integers(3, 701)), rng, *(2 * [4 * int(rng.integers(0, 4))])))
        if k in (0, nseg // 2):
            for _ in range(3):
                empty()
            null_empty.append(len(segs) - 2)
    empty()
    plan = _run(L, width, "MPI_SUM", "MPI_FLOAT", segs, null_empty)
    assert plan[2:] == (nseg, 0) and plan[1] == -(-nseg // width)


@pytest.mark.parametrize("pair", [("MPI_SUM", "MPI_FLOAT"), ("MPI_BXOR", "MPI_INT8_T")], ids=lambda p: p[0])
def test_more_than_1024_tiles_in_one_launch(L, width, pair):
    """`width` segments of 128 KiB: 32 tiles each, 4096 in one launch, so the
    launch's tile order (XCD-contiguous eighths) is a real permutation."""
    op, dt = pair
    rng = np.random.default_rng(zlib.crc32(f"tiles/{op}".encode()))
    segs = [_seg(op, dt, (128 << 10) // _esz(dt), rng) for _ in range(width)]
    assert _run(L, width, op, dt, segs)[1:] == (1, width, 0)


def test_one_large_segment_among_small_ones(L, width):
    """16 MiB + 12 bytes of fp32 SUM between small neighbours: launched on its
    own (the plan says so), right bytes, the neighbours' guards intact."""
    rng = np.random.default_rng(16)
    segs = [_seg("MPI_SUM", "MPI_FLOAT", 1000, rng), _seg("MPI_SUM", "MPI_FLOAT", 17, rng, 4, 4),
            _seg("MPI_SUM", "MPI_FLOAT", LIMIT // 4 + 3, rng), _seg("MPI_SUM", "MPI_FLOAT", 2053, rng, 12, 12),
            _seg("MPI_SUM", "MPI_FLOAT", 1, rng)]
    assert _run(L, width, "MPI_SUM", "MPI_FLOAT", segs)[1:] == (2, 4, 1)


@pytest.mark.parametrize("dt", R.TYPES)
def test_sum_wide_is_mpi_sum(L, width, dt):
    rng = np.random.default_rng(zlib.crc32(f"wide/{dt}".encode()))
    segs = [_seg("MPI_SUM", dt, n, rng, off, off) for n in (1, 9, 2047, 2049, 4105) for off in (0, 2, 14)]
    assert _run(L, width, "MSX_SUM_WIDE", dt, segs)[3] == 0


def test_stream_order_and_descriptor_capture(L, width):
    """On a non-default stream: a fill enqueued on the stream, the batch call
    on the same stream with no host synchronisation in between, the three host
    arrays zeroed as soon as the call returns, then a readback on the stream."""
    op, dt = "MPI_SUM", "MPI_FLOAT"
    rng = np.random.default_rng(33)
    n = width + 5                                  # two fused launches
    segs = [_seg(op, dt, int(rng.integers(3, 20000)), rng, *(2 * [4 * int(rng.integers(0, 4))])) for _ in range(n)]
    img_in, img_io, pin, pio = _layout(segs)
    t_in = _up(img_in)
    t_io = torch.full((img_io.size,), 0x11, dtype=torch.uint8, device="cuda")     # not the operands yet
    src = torch.from_numpy(img_io.copy()).pin_memory()
    back = torch.empty(img_io.size, dtype=torch.uint8).pin_memory()
    A = (vp * n)(*[t_in.data_ptr() + p for p in pin])
    B = (vp * n)(*[t_io.data_ptr() + p for p in pio])
    N = (i64 * n)(*[a.size // 4 for a, _, _, _ in segs])
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        t_io.copy_(src, non_blocking=True)
        rc = L.msx_reduce_local_batch_dev(A, B, N, n, h(dt), h(op), ctypes.c_void_p(s.cuda_stream))
        for arr in (A, B, N):
            ctypes.memset(arr, 0, ctypes.sizeof(arr))
        back.copy_(t_io, non_blocking=True)
    assert rc == 0, msx.last_error()
    s.synchronize()
    _same(back.numpy(), _expected(op, dt, segs, img_io, pio), segs, pio, "stream-ordered batch")
    assert np.array_equal(t_in.cpu().numpy(), img_in)


def test_a_refused_batch_writes_nothing(L):
    """The last segment's inout overlaps the first's: MPI_ERR_BUFFER naming
    both, and after a device synchronisation every inout byte is unchanged."""
    op, dt = "MPI_SUM", "MPI_FLOAT"
    rng = np.random.default_rng(34)
    segs = [_seg(op, dt, 500, rng) for _ in range(5)]
    img_in, img_io, pin, pio = _layout(segs)
    t_in, t_io = _up(img_in), _up(img_io)
    pio[4] = pio[0] + 400
    A = (vp * 5)(*[t_in.data_ptr() + p for p in pin])
    B = (vp * 5)(*[t_io.data_ptr() + p for p in pio])
    N = (i64 * 5)(*[500] * 5)
    torch.cuda.synchronize()
    assert L.msx_reduce_local_batch_dev(A, B, N, 5, h(dt), h(op), _stream()) == C.MPI_ERR_BUFFER
    err = msx.last_error()
    assert "segment 0" in err and "segment 4" in err, err
    torch.cuda.synchronize()
    assert np.array_equal(t_io.cpu().numpy(), img_io)
    assert np.array_equal(t_in.cpu().numpy(), img_in)
