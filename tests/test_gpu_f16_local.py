"""GPU: MSX_FLOAT16 / MSX_BFLOAT16 through every local reduction path, byte-exact
against the numpy definition in tests/_half_ref.py (widen exactly to fp32, one
IEEE fp32 operation, round to nearest-even; x86 NaN rule in the narrow format;
MAX / MIN return an operand's bits).  Exhaustive over one operand's 65,536 bit
patterns, ragged sizes, misaligned pointers, the DRAM-regime combine, host
operands, the op table, fused trees (which must round at every node), derived
datatypes and a derived-target accumulate.
"""
import ctypes
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import msx
import _half_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

C = msx.C
PAIRS = [(op, dt) for dt in R.TYPES for op in R.OPS]
TDT = {"MSX_FLOAT16": torch.float16, "MSX_BFLOAT16": torch.bfloat16}


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    lib = msx.init(errors_return=True)
    assert lib.msx_device_count() > 0
    return lib


def h(name):
    return getattr(C, name)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a, offset=0):
    """uint16 array -> fresh device bytes at byte `offset` (page-locked source)."""
    raw = np.frombuffer(a.tobytes(), np.uint8)
    t = torch.zeros(raw.size + offset + 64, dtype=torch.uint8, device="cuda")
    if raw.size:
        t[offset:offset + raw.size] = torch.from_numpy(raw.copy()).pin_memory().cuda()
    torch.cuda.synchronize()
    return t, t.data_ptr() + offset


def _host(t, offset, n):
    hb = torch.empty(2 * n, dtype=torch.uint8).pin_memory()
    hb.copy_(t[offset:offset + 2 * n])
    torch.cuda.synchronize()
    return np.frombuffer(bytearray(hb.numpy().tobytes()), np.uint16)


def _fail(tag, a, b, got, exp):
    bad = np.nonzero(got != exp)[0]
    i = int(bad[0])
    pytest.fail(f"{tag}: {bad.size} of {exp.size} differ; elem {i}: in={int(a[i]):#06x} inout={int(b[i]):#06x} "
                f"got={int(got[i]):#06x} exp={int(exp[i]):#06x}")


def _check_dev(L, op, dt, a, b, off_in=0, off_io=0):
    """in = a, inout = b (uint16 bit patterns)."""
    exp = R.combine(op, dt, b, a)
    ta, pa = _dev(a, off_in)
    tb, pb = _dev(b, off_io)
    rc = L.msx_reduce_local_dev(pa, pb, a.size, h(dt), h(op), _stream())
    assert rc == 0, msx.last_error()
    torch.cuda.synchronize()
    got = _host(tb, off_io, b.size)
    if not np.array_equal(got, exp):
        _fail(f"{op} {dt} n={a.size} off=({off_in},{off_io})", a, b, got, exp)
    # nothing written outside [off_io, off_io + 2n)
    assert int(tb[:off_io].count_nonzero()) == 0 and int(tb[off_io + 2 * b.size:].count_nonzero()) == 0


def _bits(rng, n):
    return rng.integers(0, 1 << 16, n, dtype=np.uint32).astype(np.uint16)


def _finite(rng, n, dt):
    """Random finite bit patterns (exponent field not all ones)."""
    x = _bits(rng, n)
    inf = 0x7C00 if dt == "MSX_FLOAT16" else 0x7F80
    nf = (x & inf) == inf
    x[nf] ^= 0x0400 if dt == "MSX_FLOAT16" else 0x0080
    return x


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_exhaustive_one_operand_against_64_partners(L, pair):
    """All 65,536 bit patterns of one operand against each of 64 partner
    patterns, in both roles: one 4,194,304-element call per (op, type, role)."""
    op, dt = pair
    every = np.tile(np.arange(1 << 16, dtype=np.uint32).astype(np.uint16), 64)
    part = np.repeat(R.partners(dt), 1 << 16)
    assert every.size == part.size == 4194304
    _check_dev(L, op, dt, every, part)      # every pattern as `in`
    _check_dev(L, op, dt, part, every)      # every pattern as `inout`


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_ragged_sizes_and_cancellation(L, pair):
    op, dt = pair
    rng = np.random.default_rng(zlib.crc32(f"ragged/{op}/{dt}".encode()))
    for n in (1, 7, 8, 9, 23, 25, 1000, 65537):
        _check_dev(L, op, dt, _bits(rng, n), _bits(rng, n))
        # near-exponent pairs: b = a ^ small, opposite signs (cancellation into subnormals)
        a = _bits(rng, n)
        b = a ^ rng.integers(0, 64, n, dtype=np.uint32).astype(np.uint16) ^ np.uint16(0x8000)
        _check_dev(L, op, dt, a, b)


@pytest.mark.parametrize("dt", R.TYPES)
def test_unaligned_and_misaligned_pointers(L, dt):
    rng = np.random.default_rng(7)
    esz = 2
    for op in ("MPI_SUM", "MPI_MAX"):
        for n in (5, 4099):
            a, b = _bits(rng, n), _bits(rng, n)
            for off_in, off_io in ((esz, esz), (0, esz), (esz * 3, 0), (8, 8)):
                _check_dev(L, op, dt, a, b, off_in, off_io)
    # k_combine_shift: every relative shift 2, 4, ..., 14 between in and inout,
    # either side of the three-vector threshold (23 / 25 elements) and a ragged larger size
    for op in R.OPS:
        for n in (23, 25, 5003):
            a, b = _bits(rng, n), _bits(rng, n)
            for shift in range(2, 16, 2):
                _check_dev(L, op, dt, a, b, shift, 0)
                _check_dev(L, op, dt, a, b, 0, shift)
            _check_dev(L, op, dt, a, b, 14, 4)


_DRAM_CHILD = r'''
import ctypes, os, sys, zlib
sys.path.insert(0, os.path.join(REPO, "microsoft-mpi_amd")); sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np, torch
import msx
import _half_ref as R
L = msx.init(errors_return=True)
s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
bad = []
for dt in R.TYPES:
    for op in R.OPS:
        rng = np.random.default_rng(zlib.crc32(f"dram/{op}/{dt}".encode()))
        for n, off in ((17, 0), (65537, 0), (40000, 8)):
            a = rng.integers(0, 1 << 16, n, dtype=np.uint32).astype(np.uint16)
            b = rng.integers(0, 1 << 16, n, dtype=np.uint32).astype(np.uint16)
            exp = R.combine(op, dt, b, a)
            ta = torch.zeros(a.nbytes + off + 64, dtype=torch.uint8, device="cuda")
            tb = torch.zeros(b.nbytes + off + 64, dtype=torch.uint8, device="cuda")
            ta[off:off + a.nbytes] = torch.from_numpy(np.frombuffer(a.tobytes(), np.uint8).copy()).pin_memory().cuda()
            tb[off:off + b.nbytes] = torch.from_numpy(np.frombuffer(b.tobytes(), np.uint8).copy()).pin_memory().cuda()
            torch.cuda.synchronize()
            rc = L.msx_reduce_local_dev(ta.data_ptr() + off, tb.data_ptr() + off, n, getattr(msx.C, dt),
                                        getattr(msx.C, op), s)
            torch.cuda.synchronize()
            got = tb[off:off + b.nbytes].cpu().numpy().tobytes()
            if rc or got != exp.tobytes():
                bad.append(f"{op} {dt} n={n} off={off} rc={rc}")
print("DRAM_BAD", len(bad), bad[:5], flush=True)
'''


def test_dram_regime_combine_kernel(L):
    """k_combine_dram for the eight (op, type) pairs: MSX_TEST_COMBINE_DRAM_MIN=0
    makes a child process route every vector-path call through it."""
    env = dict(os.environ, MSX_TEST_COMBINE_DRAM_MIN="0")
    r = subprocess.run([sys.executable, "-c", f"REPO={msx.REPO_ROOT!r}\n" + _DRAM_CHILD], capture_output=True,
                       text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("DRAM_BAD")]
    assert line and line[0].split()[1] == "0", (r.stdout + r.stderr)[-3000:]


@pytest.mark.parametrize("pinned,mode", [(False, 0), (True, 0), (True, 1), (False, 1), (False, 2), (True, 2)])
def test_mpi_reduce_local_host_operands(L, pinned, mode):
    assert L.msx_set_staging_chunk(1 << 20) == 0      # several staging chunks at the 2 MiB size
    assert L.msx_set_host_mode(mode) == 0
    try:
        rng = np.random.default_rng(11 + mode)
        for dt, op in (("MSX_BFLOAT16", "MPI_SUM"), ("MSX_FLOAT16", "MPI_PROD")):
            for n in (1001, (2 << 20) // 2):
                a, b = _bits(rng, n), _bits(rng, n)
                exp = R.combine(op, dt, b, a)
                if pinned:
                    ta = torch.from_numpy(a.view(np.uint8).copy()).pin_memory()
                    tb = torch.from_numpy(b.view(np.uint8).copy()).pin_memory()
                    rc = L.MPI_Reduce_local(ta.data_ptr(), tb.data_ptr(), n, h(dt), h(op))
                    got = np.frombuffer(tb.numpy().tobytes(), np.uint16)
                else:
                    bb = b.copy()
                    rc = L.MPI_Reduce_local(a.ctypes.data, bb.ctypes.data, n, h(dt), h(op))
                    got = bb
                assert rc == 0, msx.last_error()
                if not np.array_equal(got, exp):
                    _fail(f"host {op} {dt} n={n} pinned={pinned} mode={mode}", a, b, got, exp)
    finally:
        assert L.msx_set_staging_chunk(64 << 20) == 0
        assert L.msx_set_host_mode(0) == 0


def test_op_table_entry_on_device_operands(L):
    UF = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int),
                          ctypes.POINTER(ctypes.c_int))
    L.msx_op_table.restype = ctypes.c_void_p
    L.msx_op_table.argtypes = [ctypes.c_int]
    L.msx_op_errno.restype = ctypes.c_int
    fsum = UF(L.msx_op_table(C.MPI_SUM))
    rng = np.random.default_rng(5)
    for dt in R.TYPES:
        n = 4099
        a, b = _bits(rng, n), _bits(rng, n)
        ta, pa = _dev(a)
        tb, pb = _dev(b)
        L.msx_op_errno_reset()
        fsum(pa, pb, ctypes.byref(ctypes.c_int(n)), ctypes.byref(ctypes.c_int(h(dt))))
        assert L.msx_op_errno() == 0, msx.last_error()
        got = _host(tb, 0, n)
        exp = R.combine("MPI_SUM", dt, b, a)
        if not np.array_equal(got, exp):
            _fail(f"op table SUM {dt}", a, b, got, exp)


TREE_PAIRS = [("MPI_SUM", "MSX_BFLOAT16"), ("MPI_PROD", "MSX_FLOAT16"), ("MPI_MAX", "MSX_BFLOAT16")]


def _tree_inputs(op, dt, n, rng, k):
    srcs = [_bits(rng, n) for _ in range(k)]
    if op == "MPI_PROD":
        # keep products in range on most elements: magnitudes near 1 on half of them
        one = 0x3C00 if dt == "MSX_FLOAT16" else 0x3F80
        for s in srcs:
            near = rng.random(n) < 0.5
            s[near] = (one + rng.integers(-300, 300, int(near.sum()))).astype(np.uint16) | \
                (rng.integers(0, 2, int(near.sum())).astype(np.uint16) << 15)
    return srcs


@pytest.mark.parametrize("pair", TREE_PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_tree_folds_absent_leaves_and_chains(L, pair):
    """Every shape run_tree_sel selects (the case list of
    test_gpu_local.test_tree_folds_absent_leaves_and_chains) against the same
    tree walked with the numpy combine: the fused kernel must round at every
    node."""
    op, dt = pair
    rng = np.random.default_rng(zlib.crc32(f"spec/{op}/{dt}".encode()))
    n = 4099
    srcs = _tree_inputs(op, dt, n, rng, 16)
    devs = [_dev(x) for x in srcs]
    ptrs = [p for _, p in devs]
    cases = []
    for P in (2, 4, 8):
        for nl in range(1, P + 1):
            cases.append((P, 0, nl, 0))                        # absent leaves (binomial trees)
        for pm in range(1, 1 << P) if P < 8 else rng.integers(1, 256, 24):
            cases.append((P, int(pm), P, 0))                   # folds (pairs)
        cases.append((P, int(rng.integers(0, 1 << P)), int(rng.integers(1, P + 1)), 0))
    for P in range(2, 9):
        cases.append((P, 0, 0, 1))                             # chains
    out = torch.zeros(n * 2 + 64, dtype=torch.uint8, device="cuda")
    for P, pm, nl, chain in cases:
        ns = P if chain else 2 * P
        arr = (ctypes.c_void_p * ns)(*ptrs[:ns])
        rc = L.msx_reduce_tree_spec_dev(arr, P, pm, nl, chain, out.data_ptr(), n, h(dt), h(op), _stream())
        assert rc == 0, msx.last_error()
        torch.cuda.synchronize()
        got = _host(out, 0, n)
        exp = R.tree(op, dt, srcs[:ns], P, pm, nl, chain)
        assert np.array_equal(got, exp), (op, dt, P, hex(pm), nl, chain, int(np.count_nonzero(got != exp)))


@pytest.mark.parametrize("p", [2, 8, 16])
def test_tree_dev_balanced(L, p):
    rng = np.random.default_rng(1000 + p)
    n = 4099
    for op, dt in TREE_PAIRS:
        xs = _tree_inputs(op, dt, n, rng, p)
        dv = [_dev(x) for x in xs]
        arr = (ctypes.c_void_p * p)(*[d[1] for d in dv])
        out = torch.zeros(n * 2 + 64, dtype=torch.uint8, device="cuda")
        assert L.msx_reduce_tree_dev(arr, p, out.data_ptr(), n, h(dt), h(op), _stream()) == 0, msx.last_error()
        torch.cuda.synchronize()
        lv = [x.copy() for x in xs]
        while len(lv) > 1:
            lv = [R.combine(op, dt, lv[i], lv[i + 1]) for i in range(0, len(lv), 2)]
        assert np.array_equal(_host(out, 0, n), lv[0]), (op, dt, p)


def test_trees_dram_regime_against_torch(L):
    """The non-temporal, 64-lane tree forms (source bytes above 256 MiB): the
    8-source chain and the 8-leaf full tree.  Finite bf16 inputs, against
    torch evaluating the same association in bf16 on the GPU (one rounded bf16
    add per node)."""
    n = 17 << 20                                   # 34 MiB per source: 8 sources read 272 MiB
    dt, tdt = C.MSX_BFLOAT16, torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(6)
    xs = [(torch.rand(n, device="cuda", generator=g) * 2 - 1).to(tdt) for _ in range(8)]
    out = torch.empty_like(xs[0])
    torch.cuda.synchronize()

    def run(srcs, P, pm, nl, chain):
        arr = (ctypes.c_void_p * len(srcs))(*[x.data_ptr() for x in srcs])
        assert L.msx_reduce_tree_spec_dev(arr, P, pm, nl, chain, out.data_ptr(), n, dt, C.MPI_SUM,
                                          _stream()) == 0, msx.last_error()
        torch.cuda.synchronize()

    def same(exp, tag):
        assert torch.equal(out.view(torch.int16), exp.view(torch.int16)), tag

    run(xs, 8, 0, 0, 1)                                                   # 8-source chain
    exp = xs[0]
    for k in range(1, 8):
        exp = exp + xs[k]
    same(exp, "chain 8")
    slots = [xs[k // 2] for k in range(16)]
    run(slots, 8, 0, 8, 0)                                                # 8-leaf full tree
    same(((xs[0] + xs[1]) + (xs[2] + xs[3])) + ((xs[4] + xs[5]) + (xs[6] + xs[7])), "tree 8")
    del slots, xs, out, exp
    torch.cuda.empty_cache()


def test_dram_regime_two_pair_fold_and_binomial_large_sources(L):
    """The two cases whose sources must be larger to cross 256 MiB of reads:
    the P = 4 two-pair fold (six sources) and the 7-of-8 binomial tree (seven),
    at 24 Mi fp16 elements (48 MiB) per source."""
    n = 24 << 20
    dt, tdt = C.MSX_FLOAT16, torch.float16
    g = torch.Generator(device="cuda").manual_seed(9)
    xs = [(torch.rand(n, device="cuda", generator=g) * 2 - 1).to(tdt) for _ in range(8)]
    out = torch.empty_like(xs[0])
    torch.cuda.synchronize()
    arr = (ctypes.c_void_p * 8)(*[x.data_ptr() for x in xs])
    assert L.msx_reduce_tree_spec_dev(arr, 4, 0b11, 4, 0, out.data_ptr(), n, dt, C.MPI_SUM, _stream()) == 0, \
        msx.last_error()
    torch.cuda.synchronize()
    exp = ((xs[0] + xs[1]) + (xs[2] + xs[3])) + (xs[4] + xs[6])
    assert torch.equal(out.view(torch.int16), exp.view(torch.int16))
    arr = (ctypes.c_void_p * 16)(*[xs[k // 2].data_ptr() for k in range(16)])
    assert L.msx_reduce_tree_spec_dev(arr, 8, 0, 7, 0, out.data_ptr(), n, dt, C.MPI_SUM, _stream()) == 0, \
        msx.last_error()
    torch.cuda.synchronize()
    exp = ((xs[0] + xs[1]) + (xs[2] + xs[3])) + ((xs[4] + xs[5]) + xs[6])
    assert torch.equal(out.view(torch.int16), exp.view(torch.int16))
    del xs, out, exp
    torch.cuda.empty_cache()


def test_pack_unpack_strided_vector_of_bf16(L):
    v = ctypes.c_int()
    assert L.MPI_Type_vector(1000, 3, 5, C.MSX_BFLOAT16, ctypes.byref(v)) == 0, msx.last_error()
    assert L.MPI_Type_commit(ctypes.byref(v)) == 0
    rng = np.random.default_rng(3)
    src = _bits(rng, 1000 * 5)
    want = src.reshape(1000, 5)[:, :3].reshape(-1).copy()
    ts, ps = _dev(src)
    packed = torch.zeros(want.nbytes + 64, dtype=torch.uint8, device="cuda")
    assert L.msx_pack_dev(ps, 1, v.value, packed.data_ptr(), _stream()) == 0, msx.last_error()
    torch.cuda.synchronize()
    assert np.array_equal(_host(packed, 0, want.size), want)
    back = torch.zeros(src.nbytes + 64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert L.msx_unpack_dev(packed.data_ptr(), 1, v.value, back.data_ptr(), _stream()) == 0, msx.last_error()
    torch.cuda.synchronize()
    exp = np.zeros_like(src).reshape(1000, 5)
    exp[:, :3] = want.reshape(1000, 3)
    assert np.array_equal(_host(back, 0, src.size), exp.reshape(-1))
    # the MPI entry points on host buffers
    out = np.zeros(want.size, np.uint16)
    pos = ctypes.c_int(0)
    assert L.MPI_Pack(src.ctypes.data, 1, v.value, out.ctypes.data, out.nbytes, ctypes.byref(pos),
                      C.MPI_COMM_WORLD) == 0, msx.last_error()
    assert pos.value == want.nbytes and np.array_equal(out, want)
    un = np.zeros_like(src)
    pos = ctypes.c_int(0)
    assert L.MPI_Unpack(out.ctypes.data, out.nbytes, ctypes.byref(pos), un.ctypes.data, 1, v.value,
                        C.MPI_COMM_WORLD) == 0, msx.last_error()
    assert np.array_equal(un, exp.reshape(-1))
    assert L.MPI_Type_free(ctypes.byref(v)) == 0


def test_accumulate_on_vector_of_fp16_target_one_rank_window(L):
    """MPI_Accumulate with SUM (then MAX and REPLACE) through a vector-of-fp16
    target datatype in a one-rank window: the derived-target accumulate kernel."""
    rows, blen, stride = 700, 3, 7
    rng = np.random.default_rng(17)
    win_np = _bits(rng, rows * stride)
    org = _bits(rng, rows * blen)
    tw, pw = _dev(win_np)
    to, po = _dev(org)
    win, v = ctypes.c_int(), ctypes.c_int()
    assert L.MPI_Type_vector(rows, blen, stride, C.MSX_FLOAT16, ctypes.byref(v)) == 0
    assert L.MPI_Type_commit(ctypes.byref(v)) == 0
    assert L.MPI_Win_create(ctypes.c_void_p(pw), win_np.nbytes, 2, C.MPI_INFO_NULL, C.MPI_COMM_WORLD,
                            ctypes.byref(win)) == 0, msx.last_error()
    assert L.MPI_Win_set_errhandler(win, C.MPI_ERRORS_RETURN) == 0
    exp = win_np.copy().reshape(rows, stride)
    assert L.MPI_Win_fence(0, win) == 0
    for op in ("MPI_SUM", "MPI_MAX", "MPI_REPLACE"):
        assert L.MPI_Accumulate(ctypes.c_void_p(po), rows * blen, C.MSX_FLOAT16, 0, 0, 1, v.value, h(op),
                                win) == 0, (op, msx.last_error())
        assert L.MPI_Win_fence(0, win) == 0, msx.last_error()
        if op == "MPI_REPLACE":
            exp[:, :blen] = org.reshape(rows, blen)
        else:
            exp[:, :blen] = R.combine(op, "MSX_FLOAT16", exp[:, :blen].reshape(-1).copy(), org).reshape(rows, blen)
        torch.cuda.synchronize()
        got = _host(tw, 0, win_np.size)
        assert np.array_equal(got, exp.reshape(-1)), (op, int(np.count_nonzero(got != exp.reshape(-1))))
    # contiguous target, PROD on bf16 bits (MPI_NO_OP is not an accumulate operation)
    assert L.MPI_Accumulate(ctypes.c_void_p(po), 100, C.MSX_BFLOAT16, 0, 4, 100, C.MSX_BFLOAT16, C.MPI_PROD,
                            win) == 0, msx.last_error()
    assert L.MPI_Win_fence(0, win) == 0
    flat = exp.reshape(-1)
    flat[4:104] = R.combine("MPI_PROD", "MSX_BFLOAT16", flat[4:104].copy(), org[:100])
    torch.cuda.synchronize()
    assert np.array_equal(_host(tw, 0, win_np.size), flat)
    # MPI_Get_accumulate (MIN, then NO_OP: fetch only) and MPI_Fetch_and_op (SUM)
    res = np.zeros(100, np.uint16)
    assert L.MPI_Get_accumulate(ctypes.c_void_p(po), 100, C.MSX_BFLOAT16, res.ctypes.data, 100, C.MSX_BFLOAT16, 0,
                                200, 100, C.MSX_BFLOAT16, C.MPI_MIN, win) == 0, msx.last_error()
    assert L.MPI_Win_fence(0, win) == 0
    assert np.array_equal(res, flat[200:300])
    flat[200:300] = R.combine("MPI_MIN", "MSX_BFLOAT16", flat[200:300].copy(), org[:100])
    res2 = np.zeros(100, np.uint16)
    assert L.MPI_Get_accumulate(ctypes.c_void_p(po), 100, C.MSX_BFLOAT16, res2.ctypes.data, 100, C.MSX_BFLOAT16, 0,
                                200, 100, C.MSX_BFLOAT16, C.MPI_NO_OP, win) == 0, msx.last_error()
    one, fo = np.array([0x3C00], np.uint16), np.zeros(1, np.uint16)
    assert L.MPI_Fetch_and_op(one.ctypes.data, fo.ctypes.data, C.MSX_FLOAT16, 0, 1, C.MPI_SUM, win) == 0, \
        msx.last_error()
    assert L.MPI_Win_fence(0, win) == 0
    assert np.array_equal(res2, flat[200:300]) and fo[0] == flat[1]
    flat[1:2] = R.combine("MPI_SUM", "MSX_FLOAT16", flat[1:2].copy(), one)
    torch.cuda.synchronize()
    assert np.array_equal(_host(tw, 0, win_np.size), flat)
    assert L.MPI_Win_free(ctypes.byref(win)) == 0
    assert L.MPI_Type_free(ctypes.byref(v)) == 0
