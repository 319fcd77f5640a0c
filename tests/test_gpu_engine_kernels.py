"""GPU: the kernels the collectives run -- k_tree, k_push_wait, k_copy_segs /
k_copy_dram -- in the launch forms that only a collective reaches, driven
through the three test hooks of include/msx.h (msx_reduce_tree_done_dev,
msx_push_dev, msx_copy_segs_dev) on memory this file allocates.

The reference: trees are walked with the oracle's pairwise reduce_local
(test_gpu_local._oracle_tree; the numpy definition of tests/_half_ref.py for
the two 16-bit types), copies and pushes are the source bytes.  No tolerance:
every comparison is on bytes, and every destination is compared as a whole
IMAGE -- 64 guard bytes before and after each range included -- so a store
outside a range fails like a wrong byte inside it.

Sizes per element size (EPV = 16 / esz elements per 16-byte vector; the bitwise
ops run as uint8 over n * esz bytes, so they count in bytes): max(1, EPV - 1)
(no whole vector), EPV * 256 (exactly one 256-lane tile) and EPV * 257 + EPV - 1
(a full tile, a partial tile and a tail).  The result-ready count (count_done)
runs at 1, 31, 32, 33, 64 and 65 workgroups -- below, at and above its 32
sub-counters -- computed from run_tree's grid (ceil((nvec + tail) / 256), or
ceil(count / 256) for the all-scalar launch) and launch_push_wait's
(gx = ceil(maxbytes / 16 / 256), gx * nseg pushing workgroups).

Flags and counters are read only after torch.cuda.synchronize(): a wrong count
shows as a wrong word, never as a wait.  No hook makes a kernel wait for a flag.
"""
import ctypes
import zlib

import numpy as np
import pytest

import msx
import oracle
import _half_ref as R
from _cases import KIND, OPS, gen, h, itemsize, legal_pairs

torch = pytest.importorskip("torch")
from test_gpu_f16_local import TREE_PAIRS as HALF_TREE_PAIRS, _tree_inputs   # noqa: E402
from test_gpu_local import TREE_SPEC_PAIRS, _oracle_tree                     # noqa: E402

pytestmark = pytest.mark.gpu

C = msx.C
GUARD, FILL = 64, 0xA5
COUNT_WORDS = 1024                                    # msx_kernels.h kCountWords (32 sub-counters, kCountSubs)
NB = (1, 31, 32, 33, 64, 65)                          # workgroup counts around the 32 sub-counters
OLD = 0x1111                                          # what a flag word holds before it is posted
BITWISE = ("MPI_BAND", "MPI_BOR", "MPI_BXOR")
# C alignment of one element, per element class (the 8-byte pair types align to 4)
ALIGN = {"i1": 1, "u1": 1, "b1": 1, "i2": 2, "u2": 2, "i4": 4, "u4": 4, "i8": 8, "u8": 8, "f4": 4, "f8": 8,
         "c8": 4, "c16": 8, "ii": 4, "fi": 4, "si": 4, "di": 8, "ff": 4, "dd": 8}
# one pair per element size 1, 2, 4, 8 (alignment 4 and 8) and 16
SIZE_PAIRS = [("MPI_MIN", "MPI_INT8_T"), ("MPI_SUM", "MSX_FLOAT16"), ("MPI_SUM", "MPI_FLOAT"),
              ("MPI_MAXLOC", "MPI_SHORT_INT"), ("MPI_PROD", "MPI_C_FLOAT_COMPLEX"), ("MPI_MAX", "MPI_DOUBLE"),
              ("MPI_MINLOC", "MPI_DOUBLE_INT")]
# (P, pairmask, nleaves, chain): the fixed P = 2 tree, the masked P = 8 fold, the generic 16-leaf
# tree with pairs and absent leaves, a compile-time chain and a generic one
SHAPES = [(2, 0, 2, 0), (8, 0x25, 8, 0), (16, 0x0421, 13, 0), (5, 0, 0, 1), (11, 0, 0, 1)]


def _pid(p):
    return f"{p[0]}-{p[1]}"


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    lib = msx.init(errors_return=True)
    assert lib.msx_device_count() > 0
    return lib


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _esz(dt):
    return 2 if dt in R.TYPES else itemsize(KIND[dt])


def _align(dt):
    return 2 if dt in R.TYPES else ALIGN[KIND[dt]]


def _counts(op, esz):
    if op in BITWISE:
        return [max(1, b // esz) for b in (15, 16 * 256, 16 * 257 + 15)]
    epv = max(1, 16 // esz)
    return [max(1, epv - 1), epv * 256, epv * 257 + epv - 1]


def _inputs(op, dt, n, k, rng):
    if dt in R.TYPES:
        return _tree_inputs(op, dt, n, rng, k)
    return [np.frombuffer(bytearray(gen(KIND[dt], op, n, rng).tobytes()), gen(KIND[dt], op, 0, rng).dtype)
            for _ in range(k)]


def _ref(op, dt, srcs, P, pm, nl, chain):
    """Bytes of the tree over `srcs` (one array per kernel slot, None = unused)."""
    if dt in R.TYPES:
        return R.tree(op, dt, srcs, P, pm, nl, chain).tobytes()
    return _oracle_tree(op, dt, srcs, P, pm, nl, chain).tobytes()


class Image:
    """Byte ranges in one buffer, each with GUARD bytes of FILL on both sides
    and `off` bytes past a 16-byte boundary (the buffer's base is 256-byte
    aligned and every range's frame starts on a multiple of 256)."""

    def __init__(self):
        self.regions = []
        self.size = 0

    def add(self, nbytes, off=0):
        start = self.size + GUARD + off
        self.regions.append((start, nbytes))
        self.size = -(-(start + nbytes + GUARD) // 256) * 256
        return len(self.regions) - 1

    def host(self, datas=None):
        img = np.full(max(self.size, 256), FILL, np.uint8)
        for (start, nbytes), d in zip(self.regions, datas or []):
            if d is not None:
                assert len(d) <= nbytes
                img[start:start + len(d)] = np.frombuffer(d, np.uint8)
        return img

    def device(self, datas=None):
        if datas is None:
            t = torch.full((max(self.size, 256),), FILL, dtype=torch.uint8, device="cuda")
        else:
            t = torch.from_numpy(self.host(datas)).pin_memory().cuda()
            torch.cuda.synchronize()
        assert t.data_ptr() % 256 == 0
        return t

    def ptr(self, t, i):
        return t.data_ptr() + self.regions[i][0]

    def where(self, byte):
        for i, (start, nbytes) in enumerate(self.regions):
            if start <= byte < start + nbytes:
                return f"range {i} byte {byte - start} of {nbytes}"
            if start - GUARD <= byte < start:
                return f"{start - byte} bytes BEFORE range {i}"
            if start + nbytes <= byte < start + nbytes + GUARD:
                return f"{byte - start - nbytes} bytes PAST range {i} ({nbytes} bytes)"
        return f"padding byte {byte}"


_PIN = {}


def _back(t):
    """Device tensor -> numpy copy of its bytes, through one page-locked buffer."""
    n = t.numel() * t.element_size()
    hb = _PIN.get("b")
    if hb is None or hb.numel() < n:
        hb = _PIN["b"] = torch.empty(max(n, 1 << 20), dtype=torch.uint8).pin_memory()
    hb[:n].copy_(t.view(torch.uint8).reshape(-1))
    torch.cuda.synchronize()
    return hb[:n].numpy().copy()


def _same(img, t, datas, tag):
    got, exp = _back(t), img.host(datas)
    if not np.array_equal(got, exp):
        bad = np.nonzero(got != exp)[0]
        b = int(bad[0])
        pytest.fail(f"{tag}: {bad.size} wrong bytes, first at {img.where(b)}: got {int(got[b]):#04x} "
                    f"expected {int(exp[b]):#04x}")


def _arr(ct, vals):
    return (ct * max(1, len(vals)))(*vals)


def _run_tree(L, op, dt, ptrs, shape, out, n, extra=(), counter=None, launches=1, flags=(), seq=0):
    P, pm, nl, chain = shape
    ns = P if chain else 2 * P
    rc = L.msx_reduce_tree_done_dev(_arr(ctypes.c_void_p, list(ptrs[:ns])), P, pm, nl, chain, out,
                                    _arr(ctypes.c_void_p, list(extra)) if extra else None, len(extra), counter,
                                    launches, _arr(ctypes.c_void_p, list(flags)) if flags else None, len(flags),
                                    seq, n, h(dt), h(op), _stream())
    assert rc == 0, msx.last_error()


class Sync:
    """A zeroed counter block and flag words; check() reads them after a sync."""

    def __init__(self):
        self.counter = torch.zeros(COUNT_WORDS, dtype=torch.int32, device="cuda")
        self.words = torch.full((66,), OLD, dtype=torch.int64, device="cuda")
        self.wait = torch.zeros(2, dtype=torch.int64, device="cuda")       # the word wait_flags names
        self.err = torch.zeros(2, dtype=torch.int32, device="cuda")        # the word wait_err names

    def flags(self, n):
        self.words.fill_(OLD)
        return [self.words.data_ptr() + 8 * i for i in range(n)]

    def check(self, nposted, seq, tag, launches_counted=0):
        """Flag words [0, nposted) hold seq and the rest their old value; the
        counter block is zero (word 1 = launches_counted while a call of
        several launches is still open); the wait words are untouched."""
        w = _back(self.words).view(np.int64)
        assert (w[:nposted] == seq).all(), f"{tag}: flags {w[:nposted][w[:nposted] != seq][:4]} != seq {seq:#x}"
        assert (w[nposted:] == OLD).all(), f"{tag}: a flag word beyond the {nposted} posted changed"
        c = _back(self.counter).view(np.int32).copy()
        assert c[1] == launches_counted, f"{tag}: launch count word = {c[1]}, expected {launches_counted}"
        c[1] = 0
        nz = np.nonzero(c)[0]
        assert nz.size == 0, f"{tag}: counter word {int(nz[0])} = {int(c[nz[0]])} left non-zero ({nz.size} words)"
        assert int(_back(self.err).view(np.int32)[0]) == 0 and int(_back(self.wait).view(np.int64)[0]) == 0, tag


# ---------------------------------------------------------------------------
# a. 16-leaf patterns and long chains
# ---------------------------------------------------------------------------
def _sched(L, which, p, n):
    """(src32, P, pairmask, nleaves, chain) of msx_schedule_tree; nleaves = the
    leading leaves whose slot is not -1."""
    src = (ctypes.c_int * 32)()
    P, pm, ch = ctypes.c_int(), ctypes.c_uint(), ctypes.c_int()
    L.msx_schedule_tree.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p] * 4
    assert L.msx_schedule_tree(which, p, n, src, ctypes.byref(P), ctypes.byref(pm), ctypes.byref(ch)) == 0, \
        (which, p, n)
    src = list(src)
    if ch.value:
        return src, (P.value, 0, 0, 1)
    nl = 0
    while nl < P.value and src[2 * nl] >= 0:
        nl += 1
    return src, (P.value, pm.value, nl, 0)


def _patterns(L):
    """Every distinct (P, pairmask, nleaves) the schedules produce for p = 9..31
    -- the kernels' 16 leaves admit p <= 31 for the fold trees (allreduce,
    reduce_scatter, reduce Rabenseifner: 16 leaves of a rank or a folded pair)
    and p <= 16 for the binomial tree and the pairwise chain, which take a
    leaf / a source per rank -- plus seeded random 16-leaf patterns."""
    out, seen = [], set()

    def add(tag, src, shape):
        if shape not in seen:
            seen.add(shape)
            out.append((tag, src, shape))

    for p in range(9, 32):
        pof2 = 1 << (p.bit_length() - 1)
        for which in (0, 1, 3):
            for n in sorted({0, 3, p % pof2, pof2 - 1}):
                add(f"which={which} p={p} n={n}", *_sched(L, which, p, n))
    for p in range(9, 17):
        for root in (0, p - 1):
            add(f"binomial p={p} root={root}", *_sched(L, 4, p, root))
        add(f"chain p={p}", *_sched(L, 2, p, p // 2))
    rng = np.random.default_rng(16)
    for _ in range(6):
        nl = int(rng.integers(9, 17))
        pm = int(rng.integers(1, 1 << 16)) & ((1 << nl) - 1)
        add("random", list(range(32)), (16, pm, nl, 0))
    assert L.msx_schedule_tree(0, 32, 0, (ctypes.c_int * 32)(), ctypes.byref(ctypes.c_int()),
                               ctypes.byref(ctypes.c_uint()), ctypes.byref(ctypes.c_int())) == C.MPI_ERR_ARG
    return out


def _slots(src, shape, ptrs, xs, n):
    """Kernel-slot pointers and reference arrays of a schedule's rank table."""
    P, _, _, chain = shape
    ns = P if chain else 2 * P
    return ([ptrs[r] if r >= 0 else None for r in src[:ns]],
            [xs[r][:n] if r >= 0 else None for r in src[:ns]])


@pytest.mark.parametrize("pair", TREE_SPEC_PAIRS + HALF_TREE_PAIRS, ids=_pid)
def test_sixteen_leaf_patterns_and_long_chains(L, pair):
    """tree_eval with P = 16 and run-time pairs / absent leaves, the masked
    8-leaf folds of p = 9..15 and the chains of 9..16 sources: every pattern
    the schedules hand the kernel for 9 to 31 ranks, with rank r's vector in
    the slots the schedule names."""
    op, dt = pair
    esz = _esz(dt)
    counts = _counts(op, esz)
    rng = np.random.default_rng(zlib.crc32(f"p16/{op}/{dt}".encode()))
    xs = _inputs(op, dt, counts[-1], 32, rng)
    simg, oimg = Image(), Image()
    for x in xs:
        simg.add(x.nbytes)
    oimg.add(counts[-1] * esz)
    sdev = simg.device([x.tobytes() for x in xs])
    ptrs = [simg.ptr(sdev, i) for i in range(32)]
    pats = _patterns(L)
    assert any(s[0] == 16 and s[1] and s[2] == 16 for _, _, s in pats)      # 16-leaf folds
    assert any(s[0] == 16 and s[2] < 16 and not s[3] for _, _, s in pats)   # absent leaves
    assert {s[0] for _, _, s in pats if s[3]} == set(range(9, 17))          # chains of 9..16
    for j, (tag, src, shape) in enumerate(pats):
        for n in (counts if j % 8 == 0 or shape[3] else counts[-1:]):
            sp, sx = _slots(src, shape, ptrs, xs, n)
            out = oimg.device()
            _run_tree(L, op, dt, sp, shape, oimg.ptr(out, 0), n)
            _same(oimg, out, [_ref(op, dt, sx, *shape)], f"{op} {dt} {tag} {shape} n={n}")


@pytest.mark.parametrize("op", OPS)
def test_every_legal_pair_fold_absent_leaves_and_chain_of_11(L, op):
    """Every legal (op, type) pair through the generic kernel: p = 21's
    allreduce fold (16 leaves, five pairs), p = 11's binomial tree (16 leaves,
    five absent) and the pairwise chain of 11, at the three sizes."""
    dts = [d for o, d in legal_pairs(oracle) if o == op] + [d for d in R.TYPES if op in R.OPS]
    pats = [_sched(L, 0, 21, 5), _sched(L, 4, 11, 3), _sched(L, 2, 11, 4)]
    assert [s for _, s in pats] == [(16, pats[0][1][1], 16, 0), (16, 0, 11, 0), (11, 0, 0, 1)] and pats[0][1][1]
    for dt in dts:
        esz = _esz(dt)
        counts = _counts(op, esz)
        rng = np.random.default_rng(zlib.crc32(f"legal/{op}/{dt}".encode()))
        xs = _inputs(op, dt, counts[-1], 21, rng)
        simg, oimg = Image(), Image()
        for x in xs:
            simg.add(x.nbytes)
        for _ in range(9):
            oimg.add(counts[-1] * esz)
        sdev = simg.device([x.tobytes() for x in xs])
        ptrs = [simg.ptr(sdev, i) for i in range(21)]
        out, exp = oimg.device(), []
        for src, shape in pats:
            for n in counts:
                sp, sx = _slots(src, shape, ptrs, xs, n)
                _run_tree(L, op, dt, sp, shape, oimg.ptr(out, len(exp)), n)
                exp.append(_ref(op, dt, sx, *shape))
        _same(oimg, out, exp, f"{op} {dt} (ranges: fold, absent, chain x {counts})")


# ---------------------------------------------------------------------------
# b. misaligned trees (vec_ok == 0: the whole launch in the scalar loop)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("pair", SIZE_PAIRS, ids=_pid)
def test_misaligned_out_source_or_extra_runs_scalar(L, pair):
    """`out`, one source or the extra destination -- each in turn, then all --
    at an offset that is a multiple of the element's C alignment but not of
    16: run_tree drops the launch to the scalar loop (first = 0, nsc = tail +
    nvec * EPV).  Plain stores, one extra destination."""
    op, dt = pair
    esz, al = _esz(dt), _align(dt)
    counts = _counts(op, esz)
    rng = np.random.default_rng(zlib.crc32(f"mis/{op}/{dt}".encode()))
    xs = _inputs(op, dt, counts[-1], 32, rng)
    refs = {}
    for off in sorted({al, 16 - al}):
        assert off % al == 0 and off % 16
        simg = Image()
        for x in xs:
            simg.add(x.nbytes)
        for x in xs:
            simg.add(x.nbytes, off)
        sdev = simg.device([x.tobytes() for x in xs] * 2)
        for shape in SHAPES:
            one = 1 if shape[3] else 2                      # chain source 1 / leaf 1
            for which in ("out", "src", "extra", "all"):
                ptrs = [simg.ptr(sdev, i + (32 if which == "all" or (which == "src" and i == one) else 0))
                        for i in range(32)]
                for n in counts:
                    key = (shape, n)
                    if key not in refs:
                        refs[key] = _ref(op, dt, [x[:n] for x in xs], *shape)
                    oimg = Image()
                    oimg.add(n * esz, off if which in ("out", "all") else 0)
                    oimg.add(n * esz, off if which in ("extra", "all") else 0)
                    out = oimg.device()
                    _run_tree(L, op, dt, ptrs, shape, oimg.ptr(out, 0), n, extra=[oimg.ptr(out, 1)])
                    _same(oimg, out, [refs[key]] * 2, f"{op} {dt} {shape} n={n} off={off} misaligned={which}")


# ---------------------------------------------------------------------------
# c. extra destinations, plain stores
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("pair", SIZE_PAIRS, ids=_pid)
def test_extra_destinations_equal_out(L, pair):
    op, dt = pair
    esz = _esz(dt)
    counts = _counts(op, esz)
    rng = np.random.default_rng(zlib.crc32(f"extra/{op}/{dt}".encode()))
    xs = _inputs(op, dt, counts[-1], 32, rng)
    simg = Image()
    for x in xs:
        simg.add(x.nbytes)
    sdev = simg.device([x.tobytes() for x in xs])
    ptrs = [simg.ptr(sdev, i) for i in range(32)]
    for shape in (SHAPES[0], SHAPES[2], SHAPES[4]):
        for n in counts:
            exp = _ref(op, dt, [x[:n] for x in xs], *shape)
            for nextra in (1, 2, 31):
                oimg = Image()
                for _ in range(1 + nextra):
                    oimg.add(n * esz)
                out = oimg.device()
                _run_tree(L, op, dt, ptrs, shape, oimg.ptr(out, 0), n,
                          extra=[oimg.ptr(out, 1 + e) for e in range(nextra)])
                _same(oimg, out, [exp] * (1 + nextra), f"{op} {dt} {shape} n={n} nextra={nextra}")


# ---------------------------------------------------------------------------
# d. write-through results and the result-ready count
# ---------------------------------------------------------------------------
def _tree_grid(n, esz, vec):
    epv = 16 // esz
    nvec = n // epv
    return -(-((nvec + n - nvec * epv) if vec else n) // 256)


def _tree_count(nb, esz, vec):
    """Elements that give run_tree `nb` workgroups, with a non-empty tail
    wherever the element size leaves room for one."""
    epv = 16 // esz
    n = (256 * (nb - 1) + 1) * epv + epv - 1 if vec else 256 * (nb - 1) + 1
    assert _tree_grid(n, esz, vec) == nb and (not vec or epv == 1 or n % epv)
    return n


@pytest.mark.parametrize("pair", SIZE_PAIRS, ids=_pid)
def test_write_through_results_and_result_ready_count(L, pair):
    """With a counter the results are stored write-through (put_vec / st_wt_at
    for vectors, st_wt_elem for the tail -- and for everything when the launch
    is scalar) and the last workgroup posts the flags (tree_done, count_done).
    At 1..65 workgroups, with 0 and 3 extra destinations, one, two and 64 flag
    words, vector and scalar launches: results and extras byte-exact, every
    flag = seq, the whole counter block zero again -- and once more on the
    same block without re-zeroing it.  Destination offsets are multiples of
    the element size (what the engine's windows give); the scalar launch comes
    from a destination one element past a 16-byte boundary, or for 16-byte
    elements from a source 8 bytes past one."""
    op, dt = pair
    assert op not in BITWISE
    esz, al = _esz(dt), _align(dt)
    nmax = _tree_count(65, esz, True)
    rng = np.random.default_rng(zlib.crc32(f"wt/{op}/{dt}".encode()))
    xs = _inputs(op, dt, nmax, 16, rng) * 2         # 32 slots over 16 vectors
    simg = Image()
    for x in xs[:16]:
        simg.add(x.nbytes)
    simg.add(xs[0].nbytes, 8)                       # leaf 0 / chain source 0 again, 8 bytes off
    sdev = simg.device([x.tobytes() for x in xs[:16]] + [xs[0].tobytes()])
    ptrs = [simg.ptr(sdev, i % 16) for i in range(32)]
    sy = Sync()
    seq, i = (7 << 40) + 1, 0
    for nextra in (0, 3):
        for nb in NB:
            for vec in (True, False):
                shape, nflags = SHAPES[i % len(SHAPES)], (1, 2, 64)[i % 3]
                i += 1
                n = _tree_count(nb, esz, vec)
                doff, sp = 0, ptrs
                if not vec and esz < 16:
                    doff = esz
                elif not vec:
                    sp = [simg.ptr(sdev, 16) if s == 0 else q for s, q in enumerate(ptrs)]
                    assert al == 8
                exp = _ref(op, dt, [x[:n] for x in xs], *shape)
                oimg = Image()
                for _ in range(1 + nextra):
                    oimg.add(n * esz, doff)
                for call in range(2):                    # the second call finds the block as the first left it
                    out = oimg.device()
                    seq += 1
                    tag = f"{op} {dt} {shape} n={n} nb={nb} vec={vec} nextra={nextra} nflags={nflags} call={call}"
                    _run_tree(L, op, dt, sp, shape, oimg.ptr(out, 0), n,
                              extra=[oimg.ptr(out, 1 + e) for e in range(nextra)],
                              counter=sy.counter.data_ptr(), flags=sy.flags(nflags), seq=seq)
                    torch.cuda.synchronize()
                    _same(oimg, out, [exp] * (1 + nextra), tag)
                    sy.check(nflags, seq, tag)


@pytest.mark.parametrize("pair", [SIZE_PAIRS[2], SIZE_PAIRS[3]], ids=_pid)
def test_result_ready_flags_wait_for_the_last_of_two_launches(L, pair):
    """done_launches = 2: two launches cover two parts of one vector.  After
    the first (and a sync) the flags still hold their old value and the launch
    is counted in word 1 of the block; after the second they hold seq and the
    block is zero."""
    op, dt = pair
    esz = _esz(dt)
    epv = 16 // esz
    n = _tree_count(33, esz, True)
    rng = np.random.default_rng(zlib.crc32(f"two/{op}/{dt}".encode()))
    xs = _inputs(op, dt, n, 32, rng)
    simg = Image()
    for x in xs:
        simg.add(x.nbytes)
    sdev = simg.device([x.tobytes() for x in xs])
    sy = Sync()
    seq = (9 << 40) + 5
    for shape in (SHAPES[0], SHAPES[2]):
        exp = _ref(op, dt, xs, *shape)
        for cut in (n // 2 // epv * epv, 2 * 256 * epv, n - epv - (epv - 1)):
            assert 0 < cut < n and cut % epv == 0
            oimg = Image()
            oimg.add(n * esz)
            oimg.add(n * esz)
            out = oimg.device()
            fl = sy.flags(2)
            seq += 1
            tag = f"{op} {dt} {shape} n={n} cut={cut}"
            for lo, hi in ((0, cut), (cut, n)):
                _run_tree(L, op, dt, [simg.ptr(sdev, i) + lo * esz for i in range(32)], shape,
                          oimg.ptr(out, 0) + lo * esz, hi - lo, extra=[oimg.ptr(out, 1) + lo * esz],
                          counter=sy.counter.data_ptr(), launches=2, flags=fl, seq=seq)
                torch.cuda.synchronize()
                _same(oimg, out, [exp[:hi * esz]] * 2, f"{tag} after [{lo},{hi})")
                if hi < n:
                    sy.check(0, seq, tag + " after the first launch", launches_counted=1)
                else:
                    sy.check(2, seq, tag + " after the second launch")


# ---------------------------------------------------------------------------
# e. push (k_push_wait, copy_post_body)
# ---------------------------------------------------------------------------
LENS = (0, 1, 15, 16, 17, 4096 + 5, 2 * 4096 + 5, 3 * 4096 + 5)
# (source, destination) bytes past a 16-byte boundary: both aligned, the same
# misalignment, two different ones, and one side only
OFFS = ((0, 0), (3, 3), (5, 11), (0, 7), (9, 0), (15, 1))


def _seg_arrays(simg, sdev, dimg, ddev, segs):
    return (_arr(ctypes.c_void_p, [simg.ptr(sdev, i) for i in range(len(segs))]),
            _arr(ctypes.c_void_p, [dimg.ptr(ddev, i) for i in range(len(segs))]),
            _arr(ctypes.c_int64, [s[0] for s in segs]))


def _segments(segs, rng):
    """Images of the sources (random bytes, never FILL) and destinations of
    (nbytes, source offset, destination offset) triples."""
    simg, dimg, datas = Image(), Image(), []
    for nbytes, so, do in segs:
        simg.add(nbytes, so)
        dimg.add(nbytes, do)
        d = rng.integers(0, 255, nbytes, dtype=np.uint8)
        d[d == FILL] = 255
        datas.append(d.tobytes())
    return simg, dimg, datas


def _push(L, sy, segs, nflags, seq, rng, tag):
    simg, dimg, datas = _segments(segs, rng)
    sdev = simg.device(datas)
    for call in range(2):
        ddev = dimg.device()
        src, dst, nb = _seg_arrays(simg, sdev, dimg, ddev, segs)
        fl = sy.flags(nflags)
        rc = L.msx_push_dev(src, dst, nb, len(segs), _arr(ctypes.c_void_p, fl) if fl else None, nflags, seq + call,
                            sy.counter.data_ptr(), sy.wait.data_ptr(), sy.err.data_ptr(), _stream())
        assert rc == 0, msx.last_error()
        torch.cuda.synchronize()
        _same(dimg, ddev, datas, f"{tag} call={call}")
        sy.check(nflags, seq + call, f"{tag} call={call}")


def _push_grid(segs):
    gx = max(1, -(-(max(s[0] for s in segs) // 16) // 256))
    return gx * len(segs)


def test_push_segments_flags_and_counter(L):
    """1, 3 and 32 segments of 0 .. 3 * 4096 + 5 bytes, sources and
    destinations aligned or each 1..15 bytes off, 0, 1 and 64 flags, 1..65
    pushing workgroups; each case twice on one counter block that is never
    re-zeroed.  And the nseg = 0 form: flags, no data."""
    rng = np.random.default_rng(0xE)
    sy = Sync()
    seq, i = (3 << 40), 0
    cases = []
    for ln in LENS:
        for so, do in OFFS:
            cases.append([(ln, so, do)])
    for lens in ((17, 0, 4096 + 5), (2 * 4096 + 5, 16, 1), (15, 3 * 4096 + 5, 4096 + 5)):
        for offs in (((0, 0),) * 3, ((5, 11), (3, 3), (15, 1)), ((0, 0), (0, 7), (9, 0))):
            cases.append([(ln, so, do) for ln, (so, do) in zip(lens, offs)])
    cases.append([(LENS[k % 8], 0, 0) for k in range(32)])
    cases.append([(LENS[(k + 3) % 8], k % 16, (7 * k + 1) % 16) for k in range(32)])
    cases.append([(LENS[(5 * k) % 8], OFFS[k % 6][0], OFFS[k % 6][1]) for k in range(32)])
    grids = set()
    for nb in NB:                                                   # one segment, gx = nb
        cases.append([(4096 * (nb - 1) + 21, 0, 0)])
        cases.append([(4096 * (nb - 1) + 21, 4, 12)])
    cases.append([(4096 * 10 + 21, 0, 0), (100, 0, 0), (4096 * 10, 2, 2)])          # 3 x 11 = 33
    cases.append([(4096 + 21 if k == 9 else LENS[k % 8] % 4097, 0, k % 16) for k in range(32)])   # 32 x 2 = 64
    cases.append([(4096 * 12 + 21, 0, 0)] + [(333, 1, 0)] * 4)                      # 5 x 13 = 65
    for segs in cases:
        grids.add(_push_grid(segs))
        nflags = (0, 1, 64)[i % 3]
        i += 1
        seq += 2
        _push(L, sy, segs, nflags, seq, rng, f"push {len(segs)} segments {segs[:3]} nflags={nflags}")
    assert set(NB) <= grids, sorted(grids)
    # nseg = 0: the waiting workgroup posts the flags itself; no counter needed
    for nflags in (1, 64, 0):
        seq += 1
        fl = sy.flags(nflags)
        rc = L.msx_push_dev(None, None, None, 0, _arr(ctypes.c_void_p, fl) if fl else None, nflags, seq, None,
                            sy.wait.data_ptr(), sy.err.data_ptr(), _stream())
        assert rc == 0, msx.last_error()
        torch.cuda.synchronize()
        sy.check(nflags, seq, f"push nseg=0 nflags={nflags}")


def _dev_guarded(nbytes, off):
    """A FILL-framed device range of nbytes at `off` past a 16-byte boundary."""
    t = torch.full((GUARD + 16 + nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 16 == 0
    return t, GUARD + off


def _dev_check(t, lo, src, tag):
    n = src.numel()
    assert torch.equal(t[lo:lo + n], src), f"{tag}: data differs"
    assert bool((t[:lo] == FILL).all()) and bool((t[lo + n:] == FILL).all()), f"{tag}: bytes outside the range changed"


def test_push_four_loads_in_flight_loop(L):
    """copy_post_body's four-in-flight loop runs only when the grid is capped
    (65536 pushing workgroups over all segments): with 32 segments the stride
    is 2048 * 256 vectors = 8 MiB, so a 104 MiB + 5 B segment takes three
    passes of the unrolled loop, the one-vector loop for the rest and a byte
    tail.  The other 31 segments are short.  Compared on the device."""
    rng = np.random.default_rng(0xF)
    nbig = (104 << 20) + 5
    small = [(LENS[k % 8], k % 16, (3 * k) % 16) for k in range(31)]
    simg, dimg, datas = _segments(small, rng)
    sdev, ddev = simg.device(datas), dimg.device()
    big = torch.randint(0, 255, (nbig,), dtype=torch.uint8, device="cuda")
    bdst, lo = _dev_guarded(nbig, 0)
    assert big.data_ptr() % 16 == 0
    stride = (65536 // 32) * 256
    assert nbig // 16 > 3 * 4 * stride                     # three passes for the first lanes
    srcs = [simg.ptr(sdev, k) for k in range(31)]
    dsts = [dimg.ptr(ddev, k) for k in range(31)]
    lens = [s[0] for s in small]
    srcs.insert(17, big.data_ptr())
    dsts.insert(17, bdst.data_ptr() + lo)
    lens.insert(17, nbig)
    sy = Sync()
    fl = sy.flags(64)
    seq = (5 << 40) + 9
    rc = L.msx_push_dev(_arr(ctypes.c_void_p, srcs), _arr(ctypes.c_void_p, dsts), _arr(ctypes.c_int64, lens), 32,
                        _arr(ctypes.c_void_p, fl), 64, seq, sy.counter.data_ptr(), sy.wait.data_ptr(),
                        sy.err.data_ptr(), _stream())
    assert rc == 0, msx.last_error()
    torch.cuda.synchronize()
    _dev_check(bdst, lo, big, "104 MiB + 5 B segment")
    _same(dimg, ddev, datas, "short segments beside the long one")
    sy.check(64, seq, "push with a capped grid")


# ---------------------------------------------------------------------------
# f. copy segments and msx_copy_dev
# ---------------------------------------------------------------------------
def _copy(L, segs, rng, tag, single=False):
    simg, dimg, datas = _segments(segs, rng)
    sdev, ddev = simg.device(datas), dimg.device()
    if single:
        rc = L.msx_copy_dev(dimg.ptr(ddev, 0), simg.ptr(sdev, 0), segs[0][0], _stream())
    else:
        rc = L.msx_copy_segs_dev(*_seg_arrays(simg, sdev, dimg, ddev, segs), len(segs), _stream())
    assert rc == 0, msx.last_error()
    torch.cuda.synchronize()
    _same(dimg, ddev, datas, tag)


def test_copy_segments_tails_misalignment_and_batches(L):
    """k_copy_segs: the byte tail, the all-scalar branch for misaligned
    pointers, the workgroup % n segment mapping with unequal and empty
    segments, and the launcher's batches of 32 (33 and 70 segments: two and
    three launches); msx_copy_dev over the same lengths and misalignments."""
    rng = np.random.default_rng(0xC0)
    for ln in LENS:
        for so, do in OFFS:
            _copy(L, [(ln, so, do)], rng, f"msx_copy_dev {ln} B offsets ({so},{do})", single=True)
            _copy(L, [(ln, so, do)], rng, f"copy_segs 1 x {ln} B offsets ({so},{do})")
    for lens in ((17, 0, 4096 + 5), (2 * 4096 + 5, 16, 1), (0, 3 * 4096 + 5, 15, 0, 4096 + 5), (0, 0, 0)):
        for offs in ((0, 0), (5, 11), (0, 7)):
            _copy(L, [(ln, *offs) for ln in lens], rng, f"copy_segs {lens} offsets {offs}")
        _copy(L, [(ln, *OFFS[k % 6]) for k, ln in enumerate(lens)], rng, f"copy_segs {lens} mixed offsets")
    for nseg in (32, 33, 70):
        _copy(L, [(LENS[(3 * k) % 8], 0, 0) for k in range(nseg)], rng, f"copy_segs {nseg} aligned segments")
        _copy(L, [(LENS[(5 * k + 1) % 8], k % 16, (7 * k + 1) % 16) for k in range(nseg)], rng,
              f"copy_segs {nseg} misaligned segments")
        # the long segment in the last batch only: each batch sizes its own grid
        _copy(L, [(3 * 4096 + 5 if k == nseg - 1 else LENS[k % 5], 0, k % 2) for k in range(nseg)], rng,
              f"copy_segs {nseg} segments, the longest last")
    assert L.msx_copy_segs_dev(None, None, None, 0, _stream()) == 0


@pytest.mark.parametrize("nbytes,soff", [(16 << 20, 0), ((16 << 20) + 16, 0), ((16 << 20) + 17, 0),
                                         ((16 << 20) + 16, 8)])
def test_copy_single_segment_around_the_dram_threshold(L, nbytes, soff):
    """One segment on either side of kCopyDramMin (16 MiB) and of k_copy_dram's
    alignment condition: 16 MiB exactly stays with k_copy_segs, 16 MiB + 16
    aligned takes k_copy_dram, a ragged length or a source 8 bytes off keeps
    k_copy_segs (its vector body and byte tail, or its all-scalar branch)."""
    src, slo = _dev_guarded(nbytes, soff)
    src[slo:slo + nbytes] = torch.randint(0, 255, (nbytes,), dtype=torch.uint8, device="cuda")
    data = src[slo:slo + nbytes]
    for hook in ("msx_copy_dev", "msx_copy_segs_dev"):
        dst, dlo = _dev_guarded(nbytes, 0)
        if hook == "msx_copy_dev":
            rc = L.msx_copy_dev(dst.data_ptr() + dlo, src.data_ptr() + slo, nbytes, _stream())
        else:
            rc = L.msx_copy_segs_dev(_arr(ctypes.c_void_p, [src.data_ptr() + slo]),
                                     _arr(ctypes.c_void_p, [dst.data_ptr() + dlo]), _arr(ctypes.c_int64, [nbytes]),
                                     1, _stream())
        assert rc == 0, msx.last_error()
        torch.cuda.synchronize()
        _dev_check(dst, dlo, data, f"{hook} {nbytes} B source offset {soff}")
        del dst
