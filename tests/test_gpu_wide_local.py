"""GPU: MSX_SUM_WIDE (the fp32-accumulated tree sum of MSX_FLOAT16 /
MSX_BFLOAT16) through every local path, byte-exact against the numpy definition
in tests/_wide_ref.py: leaves widened, every node one fp32 add with the x86 NaN
rule in fp32, one narrowing at the root.

Every order-exact comparison first asserts, in numpy alone, that the wide
expectation differs from the per-node expectation of tests/_half_ref.py on the
same input: a kernel that still rounds at every node cannot pass.
"""
import ctypes
import zlib

import numpy as np
import pytest

import msx
import _half_ref as R
import _wide_ref as WR

torch = pytest.importorskip("torch")
from test_gpu_engine_kernels import COUNT_WORDS, Image, Sync, _arr, _same      # noqa: E402
from test_gpu_f16_local import _bits, _dev, _host                              # noqa: E402

pytestmark = pytest.mark.gpu

C = msx.C
TDT = {"MSX_FLOAT16": torch.float16, "MSX_BFLOAT16": torch.bfloat16}
ONE = {"MSX_FLOAT16": 0x3C00, "MSX_BFLOAT16": 0x3F80}
EPS = {"MSX_FLOAT16": 0x0C00, "MSX_BFLOAT16": 0x3B00}      # a quarter of an ulp of 1
N = 4099                                                   # 512 vectors + 3


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


def _mixed(rng, n, dt):
    """Random bit patterns (non-finite values included) at the odd indices; at
    the even ones magnitudes within a few binades of 1 with random sign and
    mantissa, so that partial sums need more mantissa than the format has and
    the per-node expectation differs from the wide one in a large share of the
    elements (bf16's exponent range makes that rare for raw random patterns)."""
    x = _bits(rng, n)
    mant = 10 if dt == "MSX_FLOAT16" else 7
    step = 2 if n >= 16 else 1             # a handful of elements: all of them near 1
    k = len(range(0, n, step))
    near = (ONE[dt] + (rng.integers(-1, 2, k) << mant) + rng.integers(0, 1 << mant, k)).astype(np.uint16)
    x[0::step] = near | (rng.integers(0, 2, k).astype(np.uint16) << 15)
    return x


def _differs(dt, srcs, P, pm, nl, chain, exp):
    """The degenerate-input guard: per-node rounding gives other bytes."""
    per_node = R.tree("MPI_SUM", dt, srcs, P, pm, nl, chain)
    assert np.count_nonzero(per_node != exp) > 0, (dt, P, hex(pm), nl, chain)


def _spec(L, dt, ptrs, P, pm, nl, chain, out_ptr, n):
    ns = P if chain else 2 * P
    arr = (ctypes.c_void_p * ns)(*ptrs[:ns])
    rc = L.msx_reduce_tree_spec_dev(arr, P, pm, nl, chain, out_ptr, n, h(dt), C.MSX_SUM_WIDE, _stream())
    assert rc == 0, msx.last_error()
    torch.cuda.synchronize()


@pytest.mark.parametrize("dt", R.TYPES)
def test_two_sources_exhaustive_equal_mpi_sum(L, dt):
    """All 65,536 patterns of one source against the 64 partners, in each role:
    widen, the NaN rule and narrow.  Over two sources the op IS MPI_SUM, so the
    expectation is checked against _half_ref.combine as well (and the
    differs-from-per-node guard does not apply)."""
    every = np.tile(np.arange(1 << 16, dtype=np.uint32).astype(np.uint16), 64)
    part = np.repeat(R.partners(dt), 1 << 16)
    assert every.size == part.size == 4194304
    for s0, s1 in ((every, part), (part, every)):
        exp = WR.balanced(dt, [s0, s1])
        assert np.array_equal(exp, R.combine("MPI_SUM", dt, s0, s1))
        (t0, p0), (t1, p1) = _dev(s0), _dev(s1)
        out = torch.zeros(2 * s0.size + 64, dtype=torch.uint8, device="cuda")
        arr = (ctypes.c_void_p * 2)(p0, p1)
        assert L.msx_reduce_tree_dev(arr, 2, out.data_ptr(), s0.size, h(dt), C.MSX_SUM_WIDE, _stream()) == 0, \
            msx.last_error()
        torch.cuda.synchronize()
        got = _host(out, 0, s0.size)
        if not np.array_equal(got, exp):
            bad = np.nonzero(got != exp)[0]
            i = int(bad[0])
            pytest.fail(f"{dt}: {bad.size} differ; elem {i}: s0={int(s0[i]):#06x} s1={int(s1[i]):#06x} "
                        f"got={int(got[i]):#06x} exp={int(exp[i]):#06x}")
        assert int(out[2 * s0.size:].count_nonzero()) == 0
        del t0, t1, out


@pytest.mark.parametrize("dt", R.TYPES)
def test_every_shape_run_tree_sel_selects(L, dt):
    """The case list of test_gpu_f16_local.test_tree_folds_absent_leaves_and_chains
    plus the chain of 9 and the 16-leaf trees (the generic kernel), random bit
    patterns with non-finite values, 4,099 elements."""
    rng = np.random.default_rng(zlib.crc32(f"wide/spec/{dt}".encode()))
    srcs = [_mixed(rng, N, dt) for _ in range(32)]
    devs = [_dev(x) for x in srcs]
    ptrs = [p for _, p in devs]
    cases = []
    for P in (2, 4, 8):
        for nl in range(1, P + 1):
            cases.append((P, 0, nl, 0))                        # absent leaves (binomial trees: 7-of-8, 5-of-8, ...)
        for pm in range(1, 1 << P) if P < 8 else rng.integers(1, 256, 24):
            cases.append((P, int(pm), P, 0))                   # folds (pairs): p = 3, 5, 6, 7, the two-pair fold
        cases.append((P, int(rng.integers(0, 1 << P)), int(rng.integers(1, P + 1)), 0))
    for P in range(2, 10):
        cases.append((P, 0, 0, 1))                             # chains 2-8 (fixed) and 9 (generic)
    cases += [(16, 0, 16, 0), (16, 0x8421, 16, 0), (16, 0x0421, 13, 0), (16, 0, 0, 1), (1, 1, 1, 0)]
    out = torch.zeros(N * 2 + 64, dtype=torch.uint8, device="cuda")
    for P, pm, nl, chain in cases:
        pm &= (1 << (nl or P)) - 1
        ns = P if chain else 2 * P
        exp = WR.tree(dt, srcs[:ns], P, pm, nl, chain)
        one_source = (chain and P == 1) or (not chain and (nl or P) == 1 and not pm & 1)
        two_sources = (chain and P == 2) or (not chain and (nl or P) + bin(pm).count("1") == 2)
        if one_source:
            assert np.array_equal(exp, srcs[0])
        elif not two_sources:
            _differs(dt, srcs[:ns], P, pm, nl, chain, exp)
        out.zero_()
        _spec(L, dt, ptrs, P, pm, nl, chain, out.data_ptr(), N)
        got = _host(out, 0, N)
        assert np.array_equal(got, exp), (dt, P, hex(pm), nl, chain, int(np.count_nonzero(got != exp)))
        assert int(out[2 * N:].count_nonzero()) == 0


@pytest.mark.parametrize("p", [2, 8, 16])
def test_tree_dev_balanced(L, p):
    rng = np.random.default_rng(2000 + p)
    for dt in R.TYPES:
        xs = [_mixed(rng, N, dt) for _ in range(p)]
        exp = WR.balanced(dt, xs)
        if p > 2:
            slots = [None] * (2 * p)
            slots[0::2] = xs
            _differs(dt, slots, p, 0, p, 0, exp)
        dv = [_dev(x) for x in xs]
        arr = (ctypes.c_void_p * p)(*[d[1] for d in dv])
        out = torch.zeros(N * 2 + 64, dtype=torch.uint8, device="cuda")
        assert L.msx_reduce_tree_dev(arr, p, out.data_ptr(), N, h(dt), C.MSX_SUM_WIDE, _stream()) == 0, \
            msx.last_error()
        torch.cuda.synchronize()
        assert np.array_equal(_host(out, 0, N), exp), (dt, p)


@pytest.mark.parametrize("dt", R.TYPES)
def test_misaligned_sources_and_destination(L, dt):
    """One source 2 bytes off: vec_ok == 0, the scalar loop.  Every source and
    `out` 2 bytes off: still no common 16-byte phase for the vector path, every
    element a head element of the scalar loop.  Counts 5 and 4,099."""
    rng = np.random.default_rng(zlib.crc32(f"wide/misaligned/{dt}".encode()))
    for n in (5, N):
        xs = [_mixed(rng, n, dt) for _ in range(8)]
        for shape in ((8, 0, 8, 0), (4, 0b0101, 4, 0), (8, 0, 5, 0), (5, 0, 0, 1), (11, 0, 0, 1)):
            P, pm, nl, chain = shape
            ns = P if chain else 2 * P
            srcs = [xs[k % 8] for k in range(ns)]
            exp = WR.tree(dt, srcs, *shape)
            _differs(dt, srcs, P, pm, nl, chain, exp)
            for offs, out_off in (([2] + [0] * 7, 0), ([2] * 8, 2)):
                devs = [_dev(x, o) for x, o in zip(xs, offs)]
                ptrs = [devs[k % 8][1] for k in range(ns)]
                out = torch.zeros(2 * n + 128, dtype=torch.uint8, device="cuda")
                _spec(L, dt, ptrs, P, pm, nl, chain, out.data_ptr() + out_off, n)
                got = _host(out, out_off, n)
                assert np.array_equal(got, exp), (dt, n, shape, offs[:2], int(np.count_nonzero(got != exp)))
                assert int(out[:out_off].count_nonzero()) == 0 and int(out[out_off + 2 * n:].count_nonzero()) == 0


@pytest.mark.parametrize("dt", R.TYPES)
def test_out_aliasing_source_zero(L, dt):
    rng = np.random.default_rng(zlib.crc32(f"wide/alias/{dt}".encode()))
    xs = [_mixed(rng, N, dt) for _ in range(8)]
    for shape in ((8, 0, 8, 0), (4, 0b0110, 4, 0), (7, 0, 0, 1), (16, 0, 9, 0)):
        P, pm, nl, chain = shape
        ns = P if chain else 2 * P
        srcs = [xs[0]] + [xs[1 + (k % 7)] for k in range(1, ns)]      # source 0 appears once
        exp = WR.tree(dt, srcs, *shape)
        _differs(dt, srcs, P, pm, nl, chain, exp)
        devs = [_dev(x) for x in xs]
        ptrs = [devs[0][1]] + [devs[1 + (k % 7)][1] for k in range(1, ns)]
        _spec(L, dt, ptrs, P, pm, nl, chain, ptrs[0], N)
        assert np.array_equal(_host(devs[0][0], 0, N), exp), (dt, shape)


def _done(L, dt, ptrs, shape, out, n, extra=(), counter=None, launches=1, flags=(), seq=0):
    P, pm, nl, chain = shape
    ns = P if chain else 2 * P
    rc = L.msx_reduce_tree_done_dev(_arr(ctypes.c_void_p, list(ptrs[:ns])), P, pm, nl, chain, out,
                                    _arr(ctypes.c_void_p, list(extra)) if extra else None, len(extra), counter,
                                    launches, _arr(ctypes.c_void_p, list(flags)) if flags else None, len(flags),
                                    seq, n, h(dt), C.MSX_SUM_WIDE, _stream())
    assert rc == 0, msx.last_error()


@pytest.mark.parametrize("dt", R.TYPES)
def test_extra_destinations_write_through_and_result_ready_count(L, dt):
    """msx_reduce_tree_done_dev: 2 and 31 extra destinations with plain stores,
    then write-through stores with the result-ready count over two launches.
    Every destination is compared as an image with its guard bytes; the counter
    block is left zero and the flags hold the sequence number only after the
    second launch."""
    rng = np.random.default_rng(zlib.crc32(f"wide/done/{dt}".encode()))
    xs = [_mixed(rng, N, dt) for _ in range(16)]
    simg = Image()
    for x in xs:
        simg.add(x.nbytes)
    sdev = simg.device([x.tobytes() for x in xs])
    ptrs = [simg.ptr(sdev, i % 16) for i in range(32)]
    sy = Sync()
    assert sy.counter.numel() == COUNT_WORDS
    seq = 0x300
    for shape in ((8, 0, 8, 0), (8, 0x25, 8, 0), (16, 0x0421, 13, 0), (5, 0, 0, 1)):
        P, pm, nl, chain = shape
        ns = P if chain else 2 * P
        srcs = [xs[i % 16] for i in range(ns)]
        exp = WR.tree(dt, srcs, *shape)
        _differs(dt, srcs, P, pm, nl, chain, exp)
        eb = exp.tobytes()
        for nextra in (2, 31):
            oimg = Image()
            for _ in range(1 + nextra):
                oimg.add(2 * N)
            # plain stores, no count
            out = oimg.device()
            _done(L, dt, ptrs, shape, oimg.ptr(out, 0), N, extra=[oimg.ptr(out, 1 + e) for e in range(nextra)])
            torch.cuda.synchronize()
            _same(oimg, out, [eb] * (1 + nextra), f"{dt} {shape} extra={nextra} plain")
            # write-through stores and the count, two launches cut at a vector boundary
            out = oimg.device()
            fl = sy.flags(3)
            seq += 1
            cut = 8 * 300
            tag = f"{dt} {shape} extra={nextra} wt"
            for lo, hi in ((0, cut), (cut, N)):
                _done(L, dt, [p + 2 * lo for p in ptrs], shape, oimg.ptr(out, 0) + 2 * lo, hi - lo,
                      extra=[oimg.ptr(out, 1 + e) + 2 * lo for e in range(nextra)], counter=sy.counter.data_ptr(),
                      launches=2, flags=fl, seq=seq)
                torch.cuda.synchronize()
                _same(oimg, out, [eb[:2 * hi]] * (1 + nextra), f"{tag} after [{lo},{hi})")
                if hi < N:
                    sy.check(0, seq, tag + " after the first launch", launches_counted=1)
                else:
                    sy.check(3, seq, tag + " after the second launch")


@pytest.mark.parametrize("dt", R.TYPES)
def test_known_answers_on_the_gpu(L, dt):
    """1 + 7 * ulp/4: 0x3F82 in bf16 (0x3C02 in fp16) as a chain and as a tree,
    where MPI_SUM's per-node rounding gives 1 (chain) and 1 + ulp (tree)."""
    srcs = [np.full(N, ONE[dt], np.uint16)] + [np.full(N, EPS[dt], np.uint16) for _ in range(7)]
    devs = [_dev(x) for x in srcs]
    out = torch.zeros(N * 2 + 64, dtype=torch.uint8, device="cuda")
    want = ONE[dt] + 2
    assert want == (0x3F82 if dt == "MSX_BFLOAT16" else 0x3C02)
    for op, chain_exp, tree_exp in ((C.MSX_SUM_WIDE, want, want), (C.MPI_SUM, ONE[dt], ONE[dt] + 1)):
        arr = (ctypes.c_void_p * 8)(*[d[1] for d in devs])
        assert L.msx_reduce_tree_spec_dev(arr, 8, 0, 0, 1, out.data_ptr(), N, h(dt), op, _stream()) == 0
        torch.cuda.synchronize()
        assert (_host(out, 0, N) == chain_exp).all()
        assert L.msx_reduce_tree_dev(arr, 8, out.data_ptr(), N, h(dt), op, _stream()) == 0
        torch.cuda.synchronize()
        assert (_host(out, 0, N) == tree_exp).all()


def test_dram_geometry_against_torch(L):
    """The non-temporal, 64-lane forms (272 MiB of sources, above kTreeNtMin):
    the 8-leaf full tree, the 8-chain and the p = 6 fold.  Finite bf16 inputs;
    torch widens to fp32, adds in the same association and rounds once."""
    n = 17 << 20
    dt, tdt = C.MSX_BFLOAT16, torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(66)
    xs = [(torch.rand(n, device="cuda", generator=g) * 2 - 1).to(tdt) for _ in range(8)]
    out = torch.empty_like(xs[0])
    torch.cuda.synchronize()

    def run(srcs, P, pm, nl, chain):
        arr = (ctypes.c_void_p * len(srcs))(*[x.data_ptr() for x in srcs])
        assert L.msx_reduce_tree_spec_dev(arr, P, pm, nl, chain, out.data_ptr(), n, dt, C.MSX_SUM_WIDE,
                                          _stream()) == 0, msx.last_error()
        torch.cuda.synchronize()

    def same(exp32, per_node, tag):
        exp = exp32.to(tdt)
        assert int((exp.view(torch.int16) != per_node.view(torch.int16)).sum()) > 0, tag      # not degenerate
        assert torch.equal(out.view(torch.int16), exp.view(torch.int16)), tag

    f = [x.float() for x in xs]
    run(xs, 8, 0, 0, 1)                                                   # 8-source chain
    e32, pn = f[0], xs[0]
    for k in range(1, 8):
        e32, pn = e32 + f[k], pn + xs[k]
    same(e32, pn, "chain 8")
    run([xs[k // 2] for k in range(16)], 8, 0, 8, 0)                      # 8-leaf full tree
    same(((f[0] + f[1]) + (f[2] + f[3])) + ((f[4] + f[5]) + (f[6] + f[7])),
         ((xs[0] + xs[1]) + (xs[2] + xs[3])) + ((xs[4] + xs[5]) + (xs[6] + xs[7])), "tree 8")
    del e32, pn
    # p = 6: four leaves, the first two folded pairs (six sources, 204 MiB: the
    # masked form with plain loads at a DRAM size) ...
    slots = [xs[0], xs[1], xs[2], xs[3], xs[4], xs[6], xs[5], xs[7]]
    run(slots, 4, 0b0011, 4, 0)
    same(((f[0] + f[1]) + (f[2] + f[3])) + (f[4] + f[5]),
         ((xs[0] + xs[1]) + (xs[2] + xs[3])) + (xs[4] + xs[5]), "fold p = 6")
    # ... and the same fold with all four pairs: eight sources, non-temporal
    run(slots, 4, 0b1111, 4, 0)
    same(((f[0] + f[1]) + (f[2] + f[3])) + ((f[4] + f[6]) + (f[5] + f[7])),
         ((xs[0] + xs[1]) + (xs[2] + xs[3])) + ((xs[4] + xs[6]) + (xs[5] + xs[7])), "fold, four pairs")
    del slots, xs, f, out
    torch.cuda.empty_cache()


def test_local_combine_equals_mpi_sum_and_float_is_refused(L):
    """One combine is MPI_SUM's: MPI_Reduce_local and msx_reduce_local_dev give
    MPI_SUM's bytes (the numpy combine) at 1,001 elements, device and host
    operands; on MPI_FLOAT both return MPI_ERR_OP and leave inout untouched."""
    rng = np.random.default_rng(77)
    n = 1001
    for dt in R.TYPES:
        a, b = _bits(rng, n), _bits(rng, n)
        exp = R.combine("MPI_SUM", dt, b, a)
        assert np.array_equal(exp, WR.tree(dt, [b, a], 2, 0, 0, 1))
        (ta, pa), (tb, pb) = _dev(a), _dev(b)
        assert L.msx_reduce_local_dev(pa, pb, n, h(dt), C.MSX_SUM_WIDE, _stream()) == 0, msx.last_error()
        torch.cuda.synchronize()
        assert np.array_equal(_host(tb, 0, n), exp), dt
        (ta, pa), (tb, pb) = _dev(a), _dev(b)
        assert L.MPI_Reduce_local(pa, pb, n, h(dt), C.MSX_SUM_WIDE) == 0, msx.last_error()
        torch.cuda.synchronize()
        assert np.array_equal(_host(tb, 0, n), exp), dt
        bb = b.copy()
        assert L.MPI_Reduce_local(a.ctypes.data, bb.ctypes.data, n, h(dt), C.MSX_SUM_WIDE) == 0, msx.last_error()
        assert np.array_equal(bb, exp), dt
        bb = b.copy()
        assert L.msx_reduce_local_multi(a.ctypes.data, bb.ctypes.data, n, h(dt), C.MSX_SUM_WIDE, 1) == 0
        assert np.array_equal(bb, exp), dt
    f = rng.random(n).astype(np.float32)
    g0 = rng.random(n).astype(np.float32)
    g = g0.copy()
    assert L.MPI_Reduce_local(f.ctypes.data, g.ctypes.data, n, C.MPI_FLOAT, C.MSX_SUM_WIDE) == C.MPI_ERR_OP
    tf = torch.from_numpy(f).cuda()
    tg = torch.from_numpy(g0).cuda()
    torch.cuda.synchronize()
    assert L.msx_reduce_local_dev(tf.data_ptr(), tg.data_ptr(), n, C.MPI_FLOAT, C.MSX_SUM_WIDE,
                                  _stream()) == C.MPI_ERR_OP
    torch.cuda.synchronize()
    assert np.array_equal(g, g0) and np.array_equal(tg.cpu().numpy(), g0)
