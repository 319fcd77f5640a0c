"""GPU: the kit's fused tree (msx_kit::tree, include/msx_device_op.h) in one
process, through msx_reduce_tree_user_dev, against the numpy evaluator of
tests/_devop_tree_ref.py (written from the header's definition of the value),
bit for bit.

Every case lays its sources and `out` into one device arena with sentinel
bytes round each of them: after the call `out` holds the expected value, every
source is unchanged (unless it is `out`) and no sentinel byte moved.  The
functor is the wrapping 3 * in - inout (+ salt), neither commutative nor
associative, so a swapped role or another association changes bits.  The ops
come from tests/devop_tree/devop_tree_ops.hip."""
import ctypes
import os

import numpy as np
import pytest

import msx
from _devop_tree_ref import devop_tree_spec, nc, tree_value

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

C = msx.C
PAD = 64            # sentinel bytes on both sides of every buffer (a multiple of 16)
SENT = 0x5A
OPS_LIB = os.path.join(msx.REPO_ROOT, "tests", "devop_tree", "build", "libdevop_tree_ops.so")
TREE_ARGS = [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
             ctypes.c_int64]


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    lib = msx.init(errors_return=True)
    assert lib.msx_device_count() > 0
    return lib


@pytest.fixture(scope="module")
def K(L):
    k = ctypes.CDLL(OPS_LIB)
    k.devop_tree_kit_u32.restype = ctypes.c_int
    k.devop_tree_kit_u32.argtypes = TREE_ARGS + [ctypes.c_int, ctypes.c_void_p]
    k.devop_tree_stats.restype = None
    k.devop_tree_stats.argtypes = [ctypes.POINTER(ctypes.c_int64), ctypes.c_int]
    return k


def _stats(K):
    """{pairwise calls, pairwise elements, tree calls, tree elements, on device, declined}; resets"""
    out = (ctypes.c_int64 * 6)()
    K.devop_tree_stats(out, 1)
    return list(out)


def _addr(K, name):
    return ctypes.cast(getattr(K, name), ctypes.c_void_p)


def _op(L, K, name, tree="", state=None, commute=0):
    op = ctypes.c_int(0)
    rc = L.msx_op_create_device_tree(_addr(K, name), _addr(K, tree or name + "_tree"), commute, state,
                                     ctypes.byref(op))
    assert rc == 0, msx.last_error()
    return op


def _record_type(L, n, base):
    t = ctypes.c_int()
    assert L.MPI_Type_contiguous(n, base, ctypes.byref(t)) == 0 and L.MPI_Type_commit(ctypes.byref(t)) == 0
    return t


@pytest.fixture(scope="module")
def ops(L, K):
    """element size -> (op, numpy dtype, numpy elements per record, MPI datatype)"""
    r16, r12 = _record_type(L, 2, C.MPI_UNSIGNED_LONG_LONG), _record_type(L, 3, C.MPI_UNSIGNED)
    table = {
        4: (_op(L, K, "devop_tree_nc_u32"), np.uint32, 1, C.MPI_UNSIGNED),
        1: (_op(L, K, "devop_tree_nc_u8"), np.uint8, 1, C.MPI_UNSIGNED_CHAR),
        2: (_op(L, K, "devop_tree_nc_u16"), np.uint16, 1, C.MPI_UNSIGNED_SHORT),
        8: (_op(L, K, "devop_tree_nc_u64"), np.uint64, 1, C.MPI_UNSIGNED_LONG_LONG),
        16: (_op(L, K, "devop_tree_nc_u64x2"), np.uint64, 2, r16.value),
        12: (_op(L, K, "devop_tree_nc_u32x3"), np.uint32, 3, r12.value),
    }
    yield table
    for op, _, _, _ in table.values():
        assert L.MPI_Op_free(ctypes.byref(op)) == 0
    assert L.MPI_Type_free(ctypes.byref(r16)) == 0 and L.MPI_Type_free(ctypes.byref(r12)) == 0


def read_slots(P, pm, nl, chain):
    """the slots a tree function may read"""
    if chain:
        return list(range(P))
    out = []
    for k in range(nl or P):
        out.append(2 * k)
        if (pm >> k) & 1:
            out.append(2 * k + 1)
    return out


class Arena:
    """One device tensor holding the read slots' buffers and, for a disjoint
    `out`, one more -- each `off[slot]` bytes from 16-byte alignment between
    sentinel bytes."""

    def __init__(self, data, out_slot, off):
        self.at = {}
        pos = 0
        keys = list(data) + ([] if out_slot is not None else ["out"])
        nbytes = next(iter(data.values())).nbytes
        for key in keys:
            self.at[key] = pos + PAD + off.get(key, off.get("all", 0))
            pos += (PAD + 16 + nbytes + PAD + 15) & ~15
        self.out_key = out_slot if out_slot is not None else "out"
        self.nbytes = nbytes
        self.host = np.full(pos, SENT, np.uint8)
        for key, a in data.items():
            self.host[self.at[key]:self.at[key] + nbytes] = np.frombuffer(a.tobytes(), np.uint8)
        self.t = torch.from_numpy(self.host.copy()).pin_memory().cuda()      # page-locked source
        torch.cuda.synchronize()                                             # the library's streams do not order after torch's
        assert self.t.data_ptr() % 16 == 0

    def ptr(self, key):
        return self.t.data_ptr() + self.at[key]

    def check(self, exp, what):
        """`out` holds exp, everything else is as it was uploaded"""
        h = torch.empty(self.t.numel(), dtype=torch.uint8).pin_memory()
        h.copy_(self.t)
        torch.cuda.synchronize()
        want = self.host.copy()
        o = self.at[self.out_key]
        if exp is not None:
            want[o:o + self.nbytes] = np.frombuffer(exp.tobytes(), np.uint8)
        bad = np.nonzero(h.numpy() != want)[0]
        assert bad.size == 0, f"{what}: {bad.size} bytes differ, first at arena byte {bad[0]} (out at {o})"


def run_case(L, ops, rng, P, pm=0, nl=0, chain=0, il=0, count=37, size=4, out_slot=None, off=None, salt=0,
             call=None, op=None, expect_rc=0):
    opv, dtype, per, mpi = ops[size]
    slots = read_slots(P, pm, nl, chain)
    data = {s: rng.integers(0, np.iinfo(dtype).max, count * per, dtype=dtype, endpoint=True) for s in slots}
    ar = Arena(data, out_slot, off or {})
    srcs = (ctypes.c_void_p * 32)()                       # slots that are not to be read stay NULL
    for s in slots:
        srcs[s] = ar.ptr(s)
    what = f"P={P} pm={pm:#x} nl={nl} chain={chain} in_left={il} count={count} size={size} out={out_slot} off={off}"
    if call is not None:
        rc = call(srcs, P, pm, nl, chain, il, ar.ptr(ar.out_key), count)
    else:
        rc = L.msx_reduce_tree_user_dev(srcs, P, pm, nl, chain, il, ar.ptr(ar.out_key), count, mpi,
                                        (op or opv).value, None)
    assert rc == expect_rc, f"{what}: rc={rc} {msx.last_error()}"
    torch.cuda.synchronize()
    exp = None
    if expect_rc == 0:
        s = [data.get(i) for i in range(32)]
        exp = tree_value(s, P, pm, nl, chain, il, lambda a, b: nc(a, b, salt))
    ar.check(exp, what)


BOTH = (0, 1)


def test_full_trees_of_every_size(L, K, ops):
    rng = np.random.default_rng(0x7EE)
    _stats(K)
    for P in (1, 2, 4, 8, 16):
        for il in BOTH:
            run_case(L, ops, rng, P, il=il, out_slot=0 if il else None)
    # one tree call of `count` elements per evaluation, no pairwise call, device memory only
    assert _stats(K) == [0, 0, 10, 10 * 37, 1, 0]


def test_every_fold_pattern_of_four_leaves(L, K, ops):
    rng = np.random.default_rng(0xF01D)
    for pm in range(16):
        for il in BOTH:
            run_case(L, ops, rng, 4, pm, il=il, out_slot=(None, 0, 2 * (pm & 3))[pm % 3])


def test_eight_leaf_folds_of_9_to_15_ranks(L, K, ops):
    """the masks the allreduce of p = 9..15 ranks hands over, at its first and last rank"""
    rng = np.random.default_rng(0x915)
    seen = set()
    for p in range(9, 16):
        for n in (0, p - 1):
            rc, _, P, pm, nl, ch, _ = devop_tree_spec(L, 0, p, n, 1, p, 4)
            assert rc == 0 and P == 8 and nl == 0 and ch == 0 and bin(pm).count("1") == p - 8
            seen.add(pm)
            for il in BOTH:
                run_case(L, ops, rng, 8, pm, il=il, out_slot=0)
    assert len(seen) >= 8


@pytest.mark.parametrize("P,nl", [(4, 3), (8, 5), (8, 6), (8, 7), (16, 9), (16, 13), (16, 15)])
def test_absent_leaves_with_and_without_pairs(L, K, ops, P, nl):
    rng = np.random.default_rng(nl)
    for pm in (0, 0b101 & ((1 << nl) - 1), (1 << nl) - 1, 1 << (nl - 1)):
        for il in BOTH:
            run_case(L, ops, rng, P, pm, nl, il=il, out_slot=(None, 0)[il])


def test_chains(L, K, ops):
    rng = np.random.default_rng(0xC4A1)
    for P in (2, 3, 8, 16):
        for il in BOTH:
            run_case(L, ops, rng, P, chain=1, il=il, out_slot=(0, P - 1)[il])
    run_case(L, ops, rng, 3, chain=1, il=0)


# a fixed-form tree with a fold, a generic-form tree with absent leaves, a chain
SHAPES = [dict(P=4, pm=0b0110), dict(P=8, pm=0b00101, nl=5), dict(P=3, chain=1)]


@pytest.mark.parametrize("count", [1, 3, 4, 5, 255, 1025, 65537])
def test_counts_round_the_vector_and_tile_sizes(L, K, ops, count):
    rng = np.random.default_rng(count)
    for i, shape in enumerate(SHAPES):
        run_case(L, ops, rng, il=(count + i) & 1, count=count, out_slot=(0, None, 1)[i], **shape)


@pytest.mark.parametrize("size", [1, 2, 8, 16, 12])
def test_every_element_size_at_a_ragged_count(L, K, ops, size):
    """12-byte records run the scalar path; the others a vector body and a tail"""
    rng = np.random.default_rng(size)
    for i, shape in enumerate(SHAPES):
        # 12-byte records 4 bytes off alignment: still on an element
        run_case(L, ops, rng, il=i & 1, count=1003, size=size, out_slot=(None, 0, 2)[i],
                 off={"all": 4} if size == 12 else None, **shape)


def test_all_pointers_offset_together_take_the_head_path(L, K, ops):
    rng = np.random.default_rng(0x4EAD)
    for i, shape in enumerate(SHAPES):
        for off in (4, 12):
            run_case(L, ops, rng, il=i & 1, count=1025, off={"all": off}, out_slot=(0, None, 0)[i], **shape)
    run_case(L, ops, rng, 4, count=2, off={"all": 4})          # shorter than the head
    run_case(L, ops, rng, 4, 0b1001, count=1027, size=2, off={"all": 6}, il=1)


def test_one_source_offset_alone_takes_the_scalar_path(L, K, ops):
    rng = np.random.default_rng(0x10E)
    run_case(L, ops, rng, 4, 0b0110, count=1025, off={3: 4}, out_slot=0)
    run_case(L, ops, rng, 8, 0b00101, 5, count=1025, off={8: 8}, il=1)
    run_case(L, ops, rng, 3, chain=1, count=1025, off={0: 4}, out_slot=0)      # `out` itself is the odd one
    run_case(L, ops, rng, 4, count=1025, off={"out": 12})


def test_out_as_any_slot_or_disjoint(L, K, ops):
    rng = np.random.default_rng(0x007)
    for il in BOTH:
        for out_slot in (0, 3, 6, None):                 # a leaf, a fold pair, the last leaf, disjoint
            run_case(L, ops, rng, 4, 0b0010, il=il, count=1029, out_slot=out_slot)
        for out_slot in (0, 5, 8, None):
            run_case(L, ops, rng, 8, 0b00100, 5, il=il, count=1029, out_slot=out_slot)
        for out_slot in (0, 2, 4, None):
            run_case(L, ops, rng, 5, chain=1, il=il, count=1029, out_slot=out_slot)


# five 256-lane tiles (twenty one-wave tiles), seven more vectors and three elements
N_TILES = 5 * 1024 + 7 * 4 + 3


@pytest.mark.parametrize("geometry", [1, 2])
def test_forced_geometry_over_several_tiles(L, K, ops, geometry):
    rng = np.random.default_rng(geometry)

    def call(*a):
        return K.devop_tree_kit_u32(*a, geometry, None)

    for i, shape in enumerate(SHAPES + [dict(P=8), dict(P=2, pm=0b11)]):
        run_case(L, ops, rng, il=i & 1, count=N_TILES, out_slot=(0, None)[i & 1], call=call, **shape)
    run_case(L, ops, rng, 4, count=N_TILES, off={2: 4}, call=call)          # the scalar path in this geometry


def test_generic_form_strides_beyond_its_grid_cap(L, K, ops):
    """more than 4096 workgroups' worth of vectors: the 256-lane generic form loops"""
    rng = np.random.default_rng(0xCA9)
    run_case(L, ops, rng, 2, chain=1, il=1, count=4096 * 256 * 4 + 4096 + 5, out_slot=0)


def test_switches_geometry_above_256_mib_of_sources(L, K, ops):
    rng = np.random.default_rng(0x256)
    run_case(L, ops, rng, 8, il=0, count=((33 << 20) + 20) // 4, out_slot=0)


def test_kit_rejects_bad_arguments(L, K):
    buf = torch.zeros(64, dtype=torch.uint8, device="cuda")
    srcs = (ctypes.c_void_p * 32)(*([buf.data_ptr()] * 32))
    out = buf.data_ptr()
    assert K.devop_tree_kit_u32(srcs, 4, 0, 0, 0, 0, out, -1, 0, None) != 0
    assert K.devop_tree_kit_u32(srcs, 4, 0, 0, 0, 0, out, 1, 3, None) != 0
    assert K.devop_tree_kit_u32(srcs, 3, 0, 0, 0, 0, out, 1, 0, None) != 0
    assert K.devop_tree_kit_u32(srcs, 4, 0, 0, 0, 2, out, 1, 0, None) != 0
    assert K.devop_tree_kit_u32(srcs, 4, 0b1000, 3, 0, 0, out, 1, 0, None) != 0
    assert K.devop_tree_kit_u32(srcs, 1, 0, 0, 1, 0, out, 1, 0, None) != 0
    srcs[2] = None
    assert K.devop_tree_kit_u32(srcs, 4, 0, 0, 0, 0, out, 1, 0, None) != 0      # a leaf that is read is NULL
    assert K.devop_tree_kit_u32(srcs, 4, 0, 0, 0, 0, out, 0, 0, None) == 0


def test_state_reaches_the_tree_function(L, K, ops):
    rng = np.random.default_rng(0x5A17)
    salt = ctypes.c_uint32(0x9E3779B9)
    op = _op(L, K, "devop_tree_nc_u32", state=ctypes.cast(ctypes.pointer(salt), ctypes.c_void_p))
    for i, shape in enumerate(SHAPES):
        run_case(L, ops, rng, il=i & 1, count=1027, off={"all": 4}, salt=salt.value, op=op, **shape)
    assert L.MPI_Op_free(ctypes.byref(op)) == 0


def test_a_decline_and_a_failure_come_back_and_write_nothing(L, K, ops):
    rng = np.random.default_rng(0xDEC)
    dec = _op(L, K, "devop_tree_nc_u32", tree="devop_tree_decline")
    bad = _op(L, K, "devop_tree_nc_u32", tree="devop_tree_fail")
    _stats(K)
    run_case(L, ops, rng, 4, 0b0011, op=dec, expect_rc=C.MSX_TREE_DECLINED)
    assert _stats(K) == [0, 0, 0, 0, 1, 1]               # the hook never falls back to the pairwise calls
    run_case(L, ops, rng, 4, 0b0011, op=bad, expect_rc=C.MPI_ERR_ARG)
    assert _stats(K) == [0, 0, 1, 0, 1, 0]
    assert L.MPI_Op_free(ctypes.byref(dec)) == 0 and L.MPI_Op_free(ctypes.byref(bad)) == 0
