"""GPU: msx_fetch_and_op_dev (k_fetch_combine / k_fetch_combine_dram,
msx_fetch.hip) against the oracle's op.cpp restatement (_half_ref.combine for
the 16-bit floats), byte for byte.

Every call's three operands are segments of three device arenas filled with a
sentinel, 64 guard bytes around every segment.  After the calls of one case:
  * the whole `inout` arena equals the expectation (the reference's combine in
    every segment, every guard byte kept);
  * the whole `fetched` arena equals the old `inout` bytes inside its
    sentinels (a pair struct's padding included);
  * the `in` arena is unchanged;
  * the same inputs through the two calls this one replaces, msx_copy_dev
    (inout -> fetched) then msx_reduce_local_dev, give the same two arenas.
One case runs sizes 1 .. 65,537 elements, each with all three operands at one
common offset off 16-byte alignment (the vector body with head and tail) and
with `fetched` at another offset (the scalar loop).  A child process with
MSX_TEST_COMBINE_DRAM_MIN=0 runs every pair again through the DRAM-regime
kernel, plus one count per element size that spans more than 1,024 one-wave
workgroups, where the XCD-run tile permutation starts to move tiles."""
import ctypes
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import msx
import oracle
import _half_ref as R
from _cases import KIND, h, legal_pairs
from test_gpu_batch_local import _data, _esz, _ref

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

C = msx.C
GUARD = 64
PAT_IN, PAT_F, PAT_IO = 0x5A, 0xC3, 0xA5
SIZES = (1, 15, 16, 17, 255, 256, 257, 4099, 65537)
BYTE_MOVERS = ("MPI_REPLACE", "MPI_NO_OP")
MOVER_TYPES = ("MPI_BYTE", "MPI_WCHAR", "MPI_FLOAT", "MPI_DOUBLE", "MPI_DOUBLE_INT", "MPI_C_DOUBLE_COMPLEX")
# 1,024 x 64 + 77 vectors: 64 whole XCD runs of the DRAM-regime grid and a cut one
BIG_VECTORS = 1024 * 64 + 77
BIG = (("MPI_SUM", "MPI_INT8_T"), ("MPI_SUM", "MSX_BFLOAT16"), ("MPI_SUM", "MPI_FLOAT"), ("MPI_SUM", "MPI_DOUBLE"),
       ("MPI_PROD", "MPI_C_DOUBLE_COMPLEX"), ("MPI_BXOR", "MPI_INT"), ("MPI_REPLACE", "MPI_WCHAR"))


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    lib = msx.init(errors_return=True)
    assert lib.msx_device_count() > 0
    return lib


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def all_pairs():
    ps = list(legal_pairs(oracle))
    ps += [(op, dt) for dt in R.TYPES for op in R.OPS] + [("MSX_SUM_WIDE", dt) for dt in R.TYPES]
    ps += [(op, dt) for op in BYTE_MOVERS for dt in MOVER_TYPES]
    return ps


def _size(dt):
    return msx.lib().msx_type_size(h(dt)) if dt not in KIND and dt not in R.TYPES else _esz(dt)


def _bytes(op, dt, n, rng):
    if op in BYTE_MOVERS:
        return rng.integers(0, 256, n * _size(dt), dtype=np.uint8)
    return _data(op, dt, n, rng)


def _expect(op, dt, a, b):
    if op == "MPI_REPLACE":
        return a
    if op == "MPI_NO_OP":
        return b
    return _ref(op, dt, a, b)


def _offsets(esz):
    """(the common offset, another one for `fetched`), both element-aligned."""
    common = esz % 16
    return common, (8 if esz >= 16 else (common + esz) % 16)


def make_segs(op, dt, sizes, tag):
    """(n, in bytes, inout bytes, off_in, off_fetched, off_inout) per size and
    placement."""
    rng = np.random.default_rng(zlib.crc32(f"fetch/{op}/{dt}/{tag}".encode()))
    common, other = _offsets(_size(dt))
    segs = []
    for n in sizes:
        for off_f in (common, other):
            segs.append((n, _bytes(op, dt, n, rng), _bytes(op, dt, n, rng), common, off_f, common))
    return segs


def _layout(segs):
    up16 = lambda v: (v + 15) // 16 * 16
    cur = [GUARD, GUARD, GUARD]
    pos = []
    for n, a, b, *offs in segs:
        p = []
        for k in range(3):
            p.append(up16(cur[k]) + offs[k])
            cur[k] = p[k] + a.size + GUARD
        pos.append(tuple(p))
    imgs = [np.full(up16(cur[k]) + 16, pat, np.uint8) for k, pat in enumerate((PAT_IN, PAT_F, PAT_IO))]
    for (n, a, b, *_), (pi, pf, po) in zip(segs, pos):
        imgs[0][pi:pi + a.size] = a
        imgs[2][po:po + b.size] = b
    return imgs, pos


def _up(img):
    t = torch.from_numpy(img.copy()).pin_memory().cuda()
    assert t.data_ptr() % 16 == 0
    return t


def _diff(got, exp, what, segs, pos, k):
    if np.array_equal(got, exp):
        return None
    i = int(np.nonzero(got != exp)[0][0])
    where = "a guard byte"
    for j, ((n, a, *_), p) in enumerate(zip(segs, pos)):
        if p[k] <= i < p[k] + a.size:
            where = f"segment {j} (n={n}, offsets {segs[j][3:]}) byte {i - p[k]}"
    return (f"{what}: {int((got != exp).sum())} bytes differ, first in {where}: "
            f"got {int(got[i]):#04x} exp {int(exp[i]):#04x}")


def check(L, op, dt, segs):
    """Run every segment through msx_fetch_and_op_dev and through the two-call
    sequence; the first discrepancy as text, or None."""
    (img_in, img_f, img_io), pos = _layout(segs)
    exp_f, exp_io = img_f.copy(), img_io.copy()
    for (n, a, b, *_), (pi, pf, po) in zip(segs, pos):
        exp_f[pf:pf + b.size] = b
        exp_io[po:po + b.size] = _expect(op, dt, a, b)
    s = _stream()
    d_in, d_f, d_io = _up(img_in), _up(img_f), _up(img_io)
    torch.cuda.synchronize()
    for (n, a, *_), (pi, pf, po) in zip(segs, pos):
        src = None if op == "MPI_NO_OP" else d_in.data_ptr() + pi
        rc = L.msx_fetch_and_op_dev(src, d_f.data_ptr() + pf, d_io.data_ptr() + po, n, h(dt), h(op), s)
        if rc != 0:
            return f"rc={rc} n={n}: {msx.last_error()}"
    torch.cuda.synchronize()
    got_f, got_io = d_f.cpu().numpy(), d_io.cpu().numpy()
    err = (_diff(got_io, exp_io, "inout", segs, pos, 2) or _diff(got_f, exp_f, "fetched", segs, pos, 1)
           or _diff(d_in.cpu().numpy(), img_in, "in", segs, pos, 0))
    if err:
        return err
    # the two calls it replaces, on fresh copies of the same arenas
    e_in, e_f, e_io = _up(img_in), _up(img_f), _up(img_io)
    torch.cuda.synchronize()
    for (n, a, *_), (pi, pf, po) in zip(segs, pos):
        pin, pf_, pio = e_in.data_ptr() + pi, e_f.data_ptr() + pf, e_io.data_ptr() + po
        rc = L.msx_copy_dev(pf_, pio, a.size, s)
        if rc == 0 and op == "MPI_REPLACE":
            rc = L.msx_copy_dev(pio, pin, a.size, s)
        elif rc == 0 and op != "MPI_NO_OP":
            rc = L.msx_reduce_local_dev(pin, pio, n, h(dt), h(op), s)
        if rc != 0:
            return f"two-call sequence rc={rc} n={n}: {msx.last_error()}"
    torch.cuda.synchronize()
    return (_diff(got_io, e_io.cpu().numpy(), "inout vs the two calls", segs, pos, 2)
            or _diff(got_f, e_f.cpu().numpy(), "fetched vs the two calls", segs, pos, 1))


def big_count(dt):
    return BIG_VECTORS * (16 // _size(dt)) + 3


# ---- every pair, every size, both placements ---------------------------------------

@pytest.mark.parametrize("pair", all_pairs(), ids=lambda p: f"{p[0]}-{p[1]}")
def test_every_pair_every_size(L, pair):
    op, dt = pair
    err = check(L, op, dt, make_segs(op, dt, SIZES, "sizes"))
    assert err is None, f"{op} {dt}: {err}"


def test_the_sweep_covers_every_element_size_and_both_bodies():
    assert {_size(dt) for _, dt in all_pairs()} >= {1, 2, 4, 8, 16}
    assert {_size(dt) for _, dt in BIG} == {1, 2, 4, 8, 16}
    for esz in (1, 2, 4, 8, 16):
        common, other = _offsets(esz)
        assert common % 16 != other % 16 and common % min(esz, 8) == 0 and other % min(esz, 8) == 0
    assert len(all_pairs()) >= 300


_DRAM_CHILD = '''
import os, sys
sys.path.insert(0, os.path.join(REPO, "microsoft-mpi_amd"))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import msx
import test_gpu_fetch_and_op as T
L = msx.init(errors_return=True)
bad = []
for op, dt in T.all_pairs():
    err = T.check(L, op, dt, T.make_segs(op, dt, T.SIZES, "dram"))
    if err:
        bad.append(f"{op} {dt}: {err}")
for op, dt in T.BIG:
    err = T.check(L, op, dt, T.make_segs(op, dt, (T.big_count(dt),), "dram-big"))
    if err:
        bad.append(f"big {op} {dt}: {err}")
print("FETCH_DRAM_BAD", len(bad), bad[:5], flush=True)
'''


def test_dram_regime_kernel_every_pair_and_past_1024_workgroups(L):
    """k_fetch_combine_dram for every pair at the same sizes and placements
    (MSX_TEST_COMBINE_DRAM_MIN=0 in a child process routes every vector-path
    call through it), and for one type of each element size one count of
    1,024 x 64 + 77 vectors plus 3 elements: the XCD-run permutation only moves
    tiles in grids above 1,024 workgroups."""
    env = dict(os.environ, MSX_TEST_COMBINE_DRAM_MIN="0")
    r = subprocess.run([sys.executable, "-c", f"REPO={msx.REPO_ROOT!r}\n" + _DRAM_CHILD], capture_output=True,
                       text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("FETCH_DRAM_BAD")]
    assert line and line[0].split()[1] == "0", (r.stdout + r.stderr)[-3000:]


# ---- NaN payloads and padding --------------------------------------------------------

F32 = np.array([0x7FC00001, 0xFFC00002, 0x7FA00003, 0xFF800000, 0x7F800000, 0x3F800000, 0x80000000, 0x00000001],
               np.uint32)
F64 = np.array([0x7FF8000000000001, 0xFFF8000000000002, 0x7FF4000000000003, 0xFFF0000000000000,
                0x7FF0000000000000, 0x3FF0000000000000, 0x8000000000000000, 1], np.uint64)


@pytest.mark.parametrize("op", ["MPI_SUM", "MPI_MAX"])
@pytest.mark.parametrize("dt", ["MPI_FLOAT", "MPI_DOUBLE", "MSX_FLOAT16", "MSX_BFLOAT16"])
def test_nan_payloads_every_partner_pair(L, dt, op):
    """Quiet and signalling NaNs with payloads, infinities of both signs, zeros
    and a subnormal, every value against every value in both roles: `fetched`
    hands back the old bit patterns untouched, `inout` the reference's."""
    vals = {"MPI_FLOAT": F32, "MPI_DOUBLE": F64}.get(dt)
    if vals is None:
        vals = R.partners(dt)
    a = np.frombuffer(np.repeat(vals, len(vals)).tobytes(), np.uint8)
    b = np.frombuffer(np.tile(vals, len(vals)).tobytes(), np.uint8)
    n = len(vals) ** 2
    common, other = _offsets(_size(dt))
    segs = [(n, a, b, common, common, common), (n, a, b, common, other, common), (n, b, a, 0, 0, 0)]
    err = check(L, op, dt, segs)
    assert err is None, err


@pytest.mark.parametrize("dt", ["MPI_DOUBLE_INT", "MPI_SHORT_INT"])
@pytest.mark.parametrize("op", ["MPI_MAXLOC", "MPI_MINLOC"])
def test_pair_struct_padding_arrives_in_fetched(L, dt, op):
    """loctype's `*this = rhs` copies the whole struct (op.cpp:327), so the
    padding of the winning operand lands in `inout`; `fetched` must carry the
    old inout's padding, whatever the op chose."""
    kind = KIND[dt]
    t = np.dtype(msx.LOC_DTYPES[kind])
    isz = t.itemsize
    pad = [i for i in range(isz) if i not in set(range(0, t["v"].itemsize)) | set(
        range(t.fields["l"][1], t.fields["l"][1] + 4))]
    assert pad
    rng = np.random.default_rng(13)
    segs = []
    for n, off_f in ((4099, 0), (257, 8)):
        a, b = _data(op, dt, n, rng).copy(), _data(op, dt, n, rng).copy()
        for p in pad:
            a[p::isz] = rng.integers(1, 256, n, dtype=np.uint8)
            b[p::isz] = rng.integers(1, 256, n, dtype=np.uint8)
        segs.append((n, a, b, 0, off_f, 0))
    err = check(L, op, dt, segs)
    assert err is None, err


# ---- the aliasing refusals ---------------------------------------------------------

def test_aliasing_is_refused_and_nothing_is_written(L):
    n = 1000
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, 4 * (4 * n + 16) + 256, dtype=np.uint8)        # in, a gap, inout, a gap
    d = _up(img)
    torch.cuda.synchronize()
    base = d.data_ptr()
    p_in, p_f, p_io = base + 64, base + 64 + 4 * n + 16, base + 64 + 2 * (4 * n + 16)
    cases = [
        (p_in, p_f, p_in, "aliases"),                       # check 5: in == inout
        (p_in, p_io, p_io, "fetched overlaps inout"),       # check 6
        (p_in, p_io + 4 * n - 4, p_io, "fetched overlaps inout"),
        (p_in, p_io - 4 * n + 4, p_io, "fetched overlaps inout"),
        (p_in, p_in + 8, p_io, "fetched overlaps in"),
    ]
    for a, f, io, text in cases:
        for op in ("MPI_SUM", "MPI_REPLACE"):
            rc = L.msx_fetch_and_op_dev(a, f, io, n, C.MPI_FLOAT, h(op), _stream())
            assert rc == C.MPI_ERR_BUFFER and text in msx.last_error(), (text, msx.last_error())
    rc = L.msx_fetch_and_op_dev(None, p_io + 8, p_io, n, C.MPI_FLOAT, C.MPI_NO_OP, _stream())
    assert rc == C.MPI_ERR_BUFFER and "fetched overlaps inout" in msx.last_error()
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), img)
    # ranges that touch end to start are legal
    rc = L.msx_fetch_and_op_dev(p_in, p_io + 4 * n, p_io, n, C.MPI_FLOAT, C.MPI_SUM, _stream())
    assert rc == 0, msx.last_error()
    torch.cuda.synchronize()
