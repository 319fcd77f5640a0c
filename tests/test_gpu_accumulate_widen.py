"""GPU: msx_accumulate_widen_dev (msx_widen.hip) against tests/_widen_ref.py,
byte for byte: W stated in integers, the combine the oracle's fp32 op.cpp
restatement with the target in the `inout` role.

Contiguous calls: the operands of one case are segments of two device arenas
filled with a sentinel, 64 guard bytes around every segment.  After the calls
the whole target arena equals the expectation (every guard byte kept) and the
origin arena is unchanged.  Layout calls: the two type maps come from
oracle/msx_dtype_oracle.py, with the arenas and helpers of
tests/test_gpu_accumulate_dev.py.  The plan (msx_accumulate_widen_plan) is
asserted before every call, so each case is known to run the path it is meant
for."""
import ctypes
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import msx
import _half_ref as R
import _widen_ref as WR
from _cases import h
from test_dtype_cpu import build_oracle, free_all
from test_gpu_accumulate_dev import _arena, _commit, _data_bytes, _same, _up
from test_gpu_batch_local import _data

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

C = msx.C
i64, c_int = ctypes.c_int64, ctypes.c_int
GUARD = 64
PAT_O, PAT_T = 0x5A, 0xA5
PAIRS = [(op, dt) for dt in WR.TYPES for op in WR.OPS]
# the 8-element work item, the 256-lane tile (2,048 elements), a third tile with head and tail
SIZES = (0, 1, 7, 8, 9, 2047, 2048, 2049, 2 * 2048 + 9)
# (origin, target) byte offsets from 16-byte alignment: a common head of 0, 1 and 7 elements (the vector body);
# two placements with no common head (element by element); origin, then target, off natural alignment (byte copies)
PLACEMENTS = ((0, 0), (14, 12), (2, 4), (2, 0), (0, 4), (1, 0), (0, 2))
# 1,024 x 64 + 77 work items: 64 whole XCD runs of the DRAM-regime grid and a cut one
BIG = (1024 * 64 + 77) * 8
# 1.0, -0.0, +inf, a quiet NaN with payload, a signalling NaN, a subnormal
TARGET_CONSTANTS = (0x3F800000, 0x80000000, 0x7F800000, 0x7FC12345, 0xFFA00001, 0x00000003)


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    lib = msx.init(errors_return=True)
    assert lib.msx_device_count() > 0
    return lib


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _plan(L, oc, odt, tc, tdt, op):
    n, path = i64(-7), c_int(-7)
    rc = L.msx_accumulate_widen_plan(oc, odt, tc, tdt, op, ctypes.byref(n), ctypes.byref(path))
    assert rc == 0, msx.last_error()
    return n.value, path.value


def _origin(op, dt, n, rng):
    return np.frombuffer(_data(op, dt, n, rng).tobytes(), np.uint16)


def _target(op, n, rng):
    return np.frombuffer(_data(op, "MPI_FLOAT", n, rng).tobytes(), np.uint32)


def make_segs(op, dt, sizes, tag, extra=3):
    """(origin uint16, target uint32, off_o, off_t) per size and placement; the
    target holds `extra` elements more than the origin."""
    rng = np.random.default_rng(zlib.crc32(f"widen/{op}/{dt}/{tag}".encode()))
    return [(_origin(op, dt, n, rng), _target(op, n + extra, rng), oo, ot) for n in sizes for oo, ot in PLACEMENTS]


def _layout(segs):
    up16 = lambda v: (v + 15) // 16 * 16
    co, ct, pos = GUARD, GUARD, []
    for a, b, oo, ot in segs:
        po, pt = up16(co) + oo, up16(ct) + ot
        co, ct = po + 2 * a.size + GUARD, pt + 4 * b.size + GUARD
        pos.append((po, pt))
    img_o, img_t = np.full(up16(co) + 16, PAT_O, np.uint8), np.full(up16(ct) + 16, PAT_T, np.uint8)
    for (a, b, *_), (po, pt) in zip(segs, pos):
        img_o[po:po + 2 * a.size] = np.frombuffer(a.tobytes(), np.uint8)
        img_t[pt:pt + 4 * b.size] = np.frombuffer(b.tobytes(), np.uint8)
    return img_o, img_t, pos


def _diff(got, exp, what, segs, pos, k):
    if np.array_equal(got, exp):
        return None
    i = int(np.nonzero(got != exp)[0][0])
    where = "a guard byte"
    for j, ((a, b, oo, ot), p) in enumerate(zip(segs, pos)):
        size = (2 * a.size, 4 * b.size)[k]
        if p[k] <= i < p[k] + size:
            where = f"segment {j} (n={a.size}, offsets {oo}, {ot}) byte {i - p[k]}"
    return (f"{what}: {int((got != exp).sum())} bytes differ, first in {where}: "
            f"got {int(got[i]):#04x} exp {int(exp[i]):#04x}")


def check(L, op, dt, segs, path=1, two_step=False):
    """Every segment through one msx_accumulate_widen_dev call; the first
    discrepancy as text, or None.  two_step: also through MPI_REPLACE into an
    fp32 scratch and msx_reduce_local_dev on MPI_FLOAT, which must agree."""
    img_o, img_t, pos = _layout(segs)
    exp = img_t.copy()
    for (a, b, *_), (po, pt) in zip(segs, pos):
        r = WR.combine(op, dt, a, b[:a.size])
        exp[pt:pt + 4 * a.size] = np.frombuffer(r.tobytes(), np.uint8)
    s = _stream()
    d_o, d_t = _up(img_o), _up(img_t)
    torch.cuda.synchronize()
    for (a, b, *_), (po, pt) in zip(segs, pos):
        want = (a.size, path if a.size else 0)
        got = _plan(L, a.size, h(dt), b.size, C.MPI_FLOAT, h(op))
        if got != want:
            return f"plan {got} != {want}"
        rc = L.msx_accumulate_widen_dev(d_o.data_ptr() + po, a.size, h(dt), d_t.data_ptr() + pt, b.size, C.MPI_FLOAT,
                                        h(op), s)
        if rc != 0:
            return f"rc={rc} n={a.size}: {msx.last_error()}"
    torch.cuda.synchronize()
    got_t = d_t.cpu().numpy()
    err = _diff(got_t, exp, "target", segs, pos, 1) or _diff(d_o.cpu().numpy(), img_o, "origin", segs, pos, 0)
    if err or not two_step:
        return err
    e_o, e_t = _up(img_o), _up(img_t)
    torch.cuda.synchronize()
    for (a, b, *_), (po, pt) in zip(segs, pos):
        if a.size == 0:
            continue
        scratch = torch.empty(a.size, dtype=torch.float32, device="cuda")
        rc = L.msx_accumulate_widen_dev(e_o.data_ptr() + po, a.size, h(dt), scratch.data_ptr(), a.size, C.MPI_FLOAT,
                                        C.MPI_REPLACE, s)
        if rc == 0:
            rc = L.msx_reduce_local_dev(scratch.data_ptr(), e_t.data_ptr() + pt, a.size, C.MPI_FLOAT, h(op), s)
        if rc != 0:
            return f"two steps rc={rc} n={a.size}: {msx.last_error()}"
        torch.cuda.synchronize()
    return _diff(got_t, e_t.cpu().numpy(), "target vs widening copy + fp32 combine", segs, pos, 1)


# ---- every pattern -------------------------------------------------------------------

@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_every_origin_pattern_against_six_target_values(L, pair):
    """All 65,536 origin patterns in one call, against each of six target
    constants.  Decides what the fp16 convert does with a signalling NaN: W
    keeps it signalling."""
    op, dt = pair
    allp = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)
    segs = [(allp, np.full(1 << 16, c, np.uint32), 0, 0) for c in TARGET_CONSTANTS]
    err = check(L, op, dt, segs)
    assert err is None, f"{op} {dt}: {err}"


# ---- sizes and placements --------------------------------------------------------------

@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_sizes_and_placements(L, pair):
    op, dt = pair
    err = check(L, op, dt, make_segs(op, dt, SIZES, "sizes"))
    assert err is None, f"{op} {dt}: {err}"


def test_the_placements_are_what_they_claim():
    def head(oo, ot):
        if oo % 2 or ot % 4:
            return "bytes"
        hs = [k for k in range(8) if (oo + 2 * k) % 16 == 0 and (ot + 4 * k) % 16 == 0]
        return hs[0] if hs else "elements"
    assert [head(*p) for p in PLACEMENTS] == [0, 1, 7, "elements", "elements", "bytes", "bytes"]


_DRAM_CHILD = '''
import os, sys
sys.path.insert(0, os.path.join(REPO, "microsoft-mpi_amd"))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import msx
import test_gpu_accumulate_widen as T
L = msx.init(errors_return=True)
bad = []
for op, dt in T.PAIRS:
    err = T.check(L, op, dt, T.make_segs(op, dt, T.SIZES, "dram"))
    if err:
        bad.append(f"{op} {dt}: {err}")
for dt in T.WR.TYPES:
    err = T.check(L, "MPI_SUM", dt, T.make_segs("MPI_SUM", dt, (T.BIG,), "dram-big")[:3])
    if err:
        bad.append(f"big MPI_SUM {dt}: {err}")
print("WIDEN_DRAM_BAD", len(bad), bad[:5], flush=True)
'''


def test_dram_regime_kernel_every_size_and_past_1024_workgroups(L):
    """k_widen_combine_dram for every pair at the same sizes and placements
    (MSX_TEST_COMBINE_DRAM_MIN=0 in a child process routes every vector-path
    call through it), and per 16-bit type one MPI_SUM of 1,024 x 64 + 77 work
    items (524,904 elements) at each common head: the XCD-run permutation only
    moves tiles in grids above 1,024 workgroups."""
    env = dict(os.environ, MSX_TEST_COMBINE_DRAM_MIN="0")
    r = subprocess.run([sys.executable, "-c", f"REPO={msx.REPO_ROOT!r}\n" + _DRAM_CHILD], capture_output=True,
                       text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("WIDEN_DRAM_BAD")]
    assert line and line[0].split()[1] == "0", (r.stdout + r.stderr)[-3000:]


# ---- against the existing fp32 kernel ------------------------------------------------------

@pytest.mark.parametrize("dt", WR.TYPES)
@pytest.mark.parametrize("op", ["MPI_SUM", "MPI_MAX"])
def test_one_call_equals_widening_copy_then_the_fp32_combine(L, op, dt):
    err = check(L, op, dt, make_segs(op, dt, (9, 2049, 65537), "two-step"), two_step=True)
    assert err is None, f"{op} {dt}: {err}"
    vals = R.partners(dt)                      # NaNs, infinities, zeros, subnormals: every origin against every target
    o = np.repeat(vals, len(vals))
    t = WR.W[dt](np.tile(vals, len(vals)))
    err = check(L, op, dt, [(o, t, 0, 0), (o, t, 2, 0)], two_step=True)
    assert err is None, f"{op} {dt}: {err}"


# ---- nothing to do ---------------------------------------------------------------------------

def test_no_op_and_zero_counts_with_null_pointers_succeed_and_write_nothing(L):
    s = _stream()
    for dt in WR.TYPES:
        assert L.msx_accumulate_widen_dev(None, 100, h(dt), None, 100, C.MPI_FLOAT, C.MPI_NO_OP, s) == 0
        for op in ("MPI_SUM", "MPI_REPLACE", "MPI_NO_OP"):
            assert L.msx_accumulate_widen_dev(None, 0, h(dt), None, 100, C.MPI_FLOAT, h(op), s) == 0
            assert L.msx_accumulate_widen_dev(None, 0, h(dt), None, 0, C.MPI_FLOAT, h(op), s) == 0
    rng = np.random.default_rng(5)
    img_o, img_t = rng.integers(0, 256, 4096, dtype=np.uint8), rng.integers(0, 256, 8192, dtype=np.uint8)
    d_o, d_t = _up(img_o), _up(img_t)
    torch.cuda.synchronize()
    assert L.msx_accumulate_widen_dev(d_o.data_ptr(), 2048, C.MSX_BFLOAT16, d_t.data_ptr(), 2048, C.MPI_FLOAT,
                                      C.MPI_NO_OP, s) == 0
    assert L.msx_accumulate_widen_dev(d_o.data_ptr(), 0, C.MSX_FLOAT16, d_t.data_ptr(), 2048, C.MPI_FLOAT,
                                      C.MPI_SUM, s) == 0
    torch.cuda.synchronize()
    assert np.array_equal(d_t.cpu().numpy(), img_t) and np.array_equal(d_o.cpu().numpy(), img_o)


# ---- layouts: the two-layout kernel ------------------------------------------------------------

BF, HF, F = ("basic", C.MSX_BFLOAT16), ("basic", C.MSX_FLOAT16), ("basic", C.MPI_FLOAT)
NAME = {C.MSX_BFLOAT16: "MSX_BFLOAT16", C.MSX_FLOAT16: "MSX_FLOAT16"}


def _eltype(rec):
    while rec[0] != "basic":
        rec = rec[-1]
    return NAME[rec[1]]


def _run(L, op, orec, ocount, trec, tcount, path=2, mis_o=0, mis_t=0):
    """One call between two layouts, checked as the module docstring says."""
    dt = _eltype(orec)
    keep = []
    oh, th = _commit(L, orec, keep), _commit(L, trec, keep)
    ot, tt = build_oracle(orec), build_oracle(trec)
    rng = np.random.default_rng(zlib.crc32(f"accw2/{op}/{orec}/{ocount}/{trec}/{tcount}".encode()))
    img_o, bo = _arena(ot, ocount, mis_o, PAT_O)
    img_t, bt = _arena(tt, tcount, mis_t, PAT_T)
    ob, tb = _data_bytes(ot, ocount, bo), _data_bytes(tt, tcount, bt)
    n = ob.size // 2
    assert ob.size % 2 == 0 and tb.size % 4 == 0 and 4 * n <= tb.size and len(set(tb.tolist())) == tb.size
    img_o[ob] = np.frombuffer(_origin(op, dt, n, rng).tobytes(), np.uint8)
    img_t[tb] = np.frombuffer(_target(op, tb.size // 4, rng).tobytes(), np.uint8)
    exp = img_t.copy()
    if op != "MPI_NO_OP":
        r = WR.combine(op, dt, np.frombuffer(img_o[ob].tobytes(), np.uint16),
                       np.frombuffer(img_t[tb[:4 * n]].tobytes(), np.uint32))
        exp[tb[:4 * n]] = np.frombuffer(r.tobytes(), np.uint8)
    assert _plan(L, ocount, oh, tcount, th, h(op)) == (n, path), (orec, trec)
    d_o, d_t = _up(img_o), _up(img_t)
    torch.cuda.synchronize()
    rc = L.msx_accumulate_widen_dev(d_o.data_ptr() + bo, ocount, oh, d_t.data_ptr() + bt, tcount, th, h(op), _stream())
    assert rc == 0, msx.last_error()
    torch.cuda.synchronize()
    tag = f"{op} {orec} x{ocount} -> {trec} x{tcount}"
    _same(d_t.cpu().numpy(), exp, tag)
    assert np.array_equal(d_o.cpu().numpy(), img_o), f"{tag}: the origin arena changed"
    free_all(L, keep)


SUB15 = ("subarray", [6, 9], [3, 5], [2, 1], True, F)                    # 15 fp32 in 3 rows of 5


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_vector_into_a_2d_subarray(L, pair):
    """MPI_Type_vector(5, 3, 7) of 16-bit floats into a 2-D fp32 subarray, 15
    elements each: 17 instances are 255 elements, 69 are 1,035."""
    op, dt = pair
    e = ("basic", h(dt))
    for count in (1, 17, 69):
        _run(L, op, ("vector", 5, 3, 7, e), count, SUB15, count)


@pytest.mark.parametrize("n", [255, 256, 257, 1029])
def test_element_counts_around_the_workgroup(L, n):
    """The 256-element tile cut and whole, both layouts strided; then a
    contiguous origin into a strided target, and the reverse."""
    col = ("subarray", [n, 4], [n, 1], [0, 2], True, F)                  # one fp32 per row of four
    _run(L, "MPI_SUM", ("vector", n, 1, 3, BF), 1, col, 1)
    _run(L, "MPI_REPLACE", ("vector", n, 1, 3, HF), 1, col, 1)
    _run(L, "MPI_MAX", HF, n, ("vector", n, 1, 3, F), 1)
    _run(L, "MPI_SUM", ("vector", n, 1, 3, BF), 1, F, n)
    _run(L, "MPI_REPLACE", ("vector", n, 1, 3, BF), 1, F, n + 5)


def test_indexed_origin_into_a_subarray(L):
    """An irregular origin (a run table on the device): 14 elements in 5 uneven
    blocks; 20 instances are 280 elements into 20 x 15, so the 19th target
    instance is partly covered and the 20th untouched."""
    ix = ("indexed", [3, 1, 4, 1, 5], [0, 5, 7, 13, 16], BF)
    for count in (1, 20):
        _run(L, "MPI_SUM", ix, count, SUB15, count)
    _run(L, "MPI_MIN", ("indexed", [3, 1, 4, 1, 5], [0, 5, 7, 13, 16], HF), 20, SUB15, 20)
    _run(L, "MPI_REPLACE", ix, 20, ("indexed", [5, 1, 4, 1, 3], [1, 8, 10, 15, 17], F), 20)


def test_partial_coverage_of_the_last_target_instance(L):
    _run(L, "MPI_SUM", ("vector", 50, 1, 2, BF), 1, ("vector", 60, 1, 3, F), 1)
    _run(L, "MPI_PROD", ("vector", 50, 1, 2, HF), 7, ("vector", 60, 1, 3, F), 6)         # 350 into 360
    _run(L, "MPI_REPLACE", ("vector", 50, 1, 2, BF), 1, ("vector", 60, 1, 3, F), 1)


@pytest.mark.parametrize("mis", [(0, 2), (1, 0), (1, 2), (0, 0)], ids=lambda m: f"o{m[0]}t{m[1]}")
def test_base_pointers_off_the_element_alignment(L, mis):
    """A target base at +2 bytes, an origin base at +1: the unaligned forms,
    whole tiles and the cut one."""
    for op, e in (("MPI_SUM", BF), ("MPI_MAX", HF), ("MPI_REPLACE", HF)):
        _run(L, op, ("vector", 2 * 256 + 1, 1, 5, e), 1, ("vector", 2 * 256 + 1, 1, 3, F), 1, 2, *mis)


def test_odd_byte_displacements_inside_the_layouts(L):
    _run(L, "MPI_SUM", ("hindexed", [2, 1, 3], [1, 15, 29], BF), 50, ("vector", 6, 1, 2, F), 50)
    _run(L, "MPI_SUM", ("vector", 6, 1, 2, HF), 50, ("hindexed", [2, 1, 3], [2, 30, 58], F), 50)


@pytest.mark.parametrize("dt", WR.TYPES)
def test_two_columns_of_one_allocation(L, dt):
    """Rows of 8 bytes in ONE allocation: a 16-bit float in bytes 0-1 of every
    row (the origin) and an fp32 in bytes 4-7 (the target).  The spans
    interleave row by row; the maps are disjoint."""
    rows = 3 * 256 + 5
    keep = []
    oh = _commit(L, ("hvector", rows, 1, 8, ("basic", h(dt))), keep)
    th = _commit(L, ("hvector", rows, 1, 8, F), keep)
    rng = np.random.default_rng(17)
    img = rng.integers(0, 256, rows * 8, dtype=np.uint8)
    m = img.reshape(rows, 8)
    m[:, 0:2] = np.frombuffer(_origin("MPI_SUM", dt, rows, rng).tobytes(), np.uint8).reshape(rows, 2)
    m[:, 4:8] = np.frombuffer(_target("MPI_SUM", rows, rng).tobytes(), np.uint8).reshape(rows, 4)
    exp = img.copy().reshape(rows, 8)
    r = WR.combine("MPI_SUM", dt, np.frombuffer(m[:, 0:2].tobytes(), np.uint16),
                   np.frombuffer(m[:, 4:8].tobytes(), np.uint32))
    exp[:, 4:8] = np.frombuffer(r.tobytes(), np.uint8).reshape(rows, 4)
    assert _plan(L, 1, oh, 1, th, C.MPI_SUM) == (rows, 2)
    d = _up(img)
    torch.cuda.synchronize()
    rc = L.msx_accumulate_widen_dev(d.data_ptr(), 1, oh, d.data_ptr() + 4, 1, th, C.MPI_SUM, _stream())
    assert rc == 0, msx.last_error()
    torch.cuda.synchronize()
    _same(d.cpu().numpy(), exp.ravel(), f"columns {dt}")
    free_all(L, keep)


def test_no_op_between_layouts_writes_nothing(L):
    _run(L, "MPI_NO_OP", ("vector", 5, 3, 7, BF), 3, SUB15, 3, 0)
