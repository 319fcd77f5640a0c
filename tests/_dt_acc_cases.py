"""The case table of the derived-target accumulate kernel (k_dt_acc_tile,
msx_pack.hip), shared by tests/test_gpu_dt_accumulate.py (which runs every
case on the GPU) and tests/test_dt_accumulate_cases_cpu.py (which checks the
table itself and every case's plan without one).

Every case is one msx_accumulate_dev call on path 2: a contiguous origin of n
basic elements into whole instances of a derived target.  The kernel has four
forms per (op, element type): REG (the magic-division map of a regular layout,
or the run table's binary search) times ALIGNED (element loads, or byte
copies).  `form` and `nruns` state what a case's target is meant to be:

  "regular"   one level: every run the same length, at one stride
  "regular2"  two levels (n1 rows at `stride`, repeated at `stride2`)
  "table"     anything else: the run table

layout_of() restates, from the oracle's type map, the merge rule of push_run
and the regularity test of build_dev_layout (msx_dtype.cpp), so the CPU test
can hold each case to its stated form."""
import zlib
from collections import namedtuple

import numpy as np

import msx
import _half_ref as R
from _cases import KIND, _float_edges, h, np_dtype
from test_dtype_cpu import build_oracle
from test_gpu_accumulate_dev import W, _pairs
from test_gpu_batch_local import _data, _esz

C = msx.C

Case = namedtuple("Case", "id sec op dt edt n trec tcount path mis_o mis_t data form nruns")
# sec: the issue's section (1-4); dt: the element datatype's name, None for
# MPI_REPLACE / MPI_NO_OP (random bytes); edt: the element datatype's name in
# either case; n: origin elements (the origin is n x ("basic", h(edt)));
# data: None (the generators of _cases) or a key of OPERANDS (section 2).

LB, UB = ("basic", C.MPI_LB), ("basic", C.MPI_UB)


def E(dt):
    return ("basic", h(dt))


def case(id, sec, op, dt, n, trec, tcount, form, nruns, path=2, mis=(0, 0), data=None, edt=None):
    return Case(id, sec, op, dt, edt or dt, n, trec, tcount, path, mis[0], mis[1], data, form, nruns)


# ---- what a recipe's layout is ------------------------------------------------------

def runs_of(t):
    """One instance's byte runs (disp, len) in type-map order, neighbours merged
    when the next element starts where the last run ends (push_run)."""
    out = []
    for d, s in t.typemap:
        if out and out[-1][0] + out[-1][1] == d:
            out[-1][1] += s
        else:
            out.append([d, s])
    return [tuple(r) for r in out]


def _uniform(runs):
    return (len({l for _, l in runs}) == 1
            and len({b[0] - a[0] for a, b in zip(runs, runs[1:])}) <= 1)


def layout_of(t):
    """(form, nruns) of an oracle type.  Two levels: the runs split into equal
    rows, each row uniform with the same length and stride, the rows' first
    runs at one stride (what a compact vector-of-vector or subarray keeps)."""
    runs = runs_of(t)
    n = len(runs)
    if _uniform(runs):
        return "regular", n
    for n1 in range(2, n // 2 + 1):
        if n % n1:
            continue
        rows = [runs[k:k + n1] for k in range(0, n, n1)]
        shape = {(r[0][1], r[1][0] - r[0][0]) for r in rows}
        if all(_uniform(r) for r in rows) and len(shape) == 1 and _uniform([r[0] for r in rows]):
            return "regular2", n
    return "table", n


# ---- section 1: every (op, element kind) in all four forms --------------------------

def IX(e):
    """The uneven five-block shape of test_gpu_accumulate_dev.IX on element e."""
    return ("indexed", [3, 1, 4, 1, 5], [0, 5, 7, 13, 16], e)


IX_COUNT = 19                    # 19 x 14 = 266 elements: ten live lanes in the second tile
MIS_U = (1, 3)                   # packed stream and typed base both off every alignment above 1


def four_forms(dt):
    """(tag, target recipe, target count, n, form, nruns, (mis_o, mis_t)) of the
    kernel's four forms.  A 1-byte element has alignof(T) = 1: no address is
    unaligned for it, so the two unaligned forms cannot be selected and are
    left out."""
    e = E(dt)
    reg = (("vector", W + 1, 1, 3, e), 1, W + 1, "regular", W + 1)
    tab = (IX(e), IX_COUNT, 14 * IX_COUNT, "table", 5)
    out = [("reg-a",) + reg + ((0, 0),), ("tab-a",) + tab + ((0, 0),)]
    if _esz(dt) > 1:
        out += [("reg-u",) + reg + (MIS_U,), ("tab-u",) + tab + (MIS_U,)]
    return out


def _forms_of(sec, prefix, op, dt, data=None):
    return [case(f"{prefix}-{tag}", sec, op, dt, n, trec, tcount, form, nruns, mis=mis, data=data)
            for tag, trec, tcount, n, form, nruns, mis in four_forms(dt)]


def pair_cases(pair):
    return _forms_of(1, f"s1-{pair[0]}-{pair[1]}", pair[0], pair[1])


def section1():
    return [c for p in _pairs() for c in pair_cases(p)]


# ---- section 2: operand order, directed ----------------------------------------------

def _nan(ft, sign, quiet, payload):
    bits, mant, u = (32, 23, np.uint32) if np.dtype(ft).itemsize == 4 else (64, 52, np.uint64)
    v = (sign << (bits - 1)) | (((1 << (bits - 1 - mant)) - 1) << mant) | (int(quiet) << (mant - 1)) | payload
    return np.array([v], u).view(ft)


def _float_operands(dt):
    """_float_edges and two more NaNs: a positive signalling one and a negative
    quiet one, with payloads of their own (bit patterns, never converted)."""
    ft = np_dtype(KIND[dt])
    return np.concatenate([_float_edges(ft), _nan(ft, 0, False, 0x123), _nan(ft, 1, True, 0x456)])


# +-0, +-inf, a quiet NaN of either sign, two signalling NaNs, the smallest
# subnormal, the smallest normal, the largest finite of either sign, +-1, 1 + ulp
_HALF_PICK = [0, 1, 2, 3, 4, 5, 6, 7, 10, 14, 16, 17, 18, 19, 20]


def _half_operands(dt):
    return R.partners(dt)[_HALF_PICK]


def _loc_operands(dt):
    """Equal values with differing locations (and one exact repeat), so the
    cross product holds every tie in both orders; NaN, +-0 and inf values for
    the float kind."""
    if KIND[dt] == "ii":
        p = [(0, 5), (0, 2), (0, 9), (1, 5), (1, 1), (-1, 7), (-1, 7), (-2 ** 31, 3), (2 ** 31 - 1, -4)]
    else:
        nan = float("nan")
        p = [(0.0, 5), (0.0, 2), (-0.0, 3), (1.0, 5), (1.0, 1), (nan, 4), (nan, 8), (-1.0, 7), (-1.0, 7),
             (float("inf"), 0), (float("-inf"), 6)]
    return np.array(p, dtype=np_dtype(KIND[dt]))


OPERANDS = {"float": _float_operands, "half": _half_operands, "loc": _loc_operands}
DIRECTED = ([(op, dt, "float") for dt in ("MPI_FLOAT", "MPI_DOUBLE") for op in ("MPI_SUM", "MPI_PROD", "MPI_MAX", "MPI_MIN")]
            + [(op, dt, "half") for dt in R.TYPES for op in R.OPS]
            + [(op, dt, "loc") for dt in ("MPI_2REAL", "MPI_2INT") for op in ("MPI_MAXLOC", "MPI_MINLOC")])


def cross(vals):
    """Origin and target operands of the full ordered cross product."""
    return np.repeat(vals, len(vals)), np.tile(vals, len(vals))


def directed_cases(entry):
    op, dt, key = entry
    return _forms_of(2, f"s2-{op}-{dt}", op, dt, data=key)


def section2():
    return [c for e in DIRECTED for c in directed_cases(e)]


def operands(c):
    """(origin bytes, target bytes) of a directed case: the cross product of
    OPERANDS[c.data](c.dt), origin value major, then _data's values up to n."""
    o, t = cross(OPERANDS[c.data](c.dt))
    pad = c.n - o.size
    assert pad >= 0
    rng = np.random.default_rng(zlib.crc32(c.id.encode()))
    return tuple(np.concatenate([np.frombuffer(x.tobytes(), np.uint8), _data(c.op, c.dt, pad, rng)]) for x in (o, t))


# ---- section 3: tile edges -----------------------------------------------------------

EDGE_NS = (1, 63, 64, 65, W - 1, W, W + 1, 3 * W + 5)
TRIPLE = (("MPI_SUM", "MPI_FLOAT"), ("MPI_BXOR", "MPI_INT16_T"), ("MPI_PROD", "MPI_C_DOUBLE_COMPLEX"))


def cycle_blocks(n):
    """Block lengths cycling 1, 2, 3 (the last cut) that total n elements, and
    their displacements with one-element gaps."""
    blens, disps, at = [], [], 0
    while sum(blens) < n:
        b = min((1, 2, 3)[len(blens) % 3], n - sum(blens))
        blens.append(b)
        disps.append(at)
        at += b + 1
    return blens, disps


def section3():
    """n = 1 is a one-run target whose first run holds the whole origin, so
    msx_accumulate_dev hands it to msx_reduce_local_dev: the plan says path 1,
    and the case states that.  The kernel's one-element launch is reached
    through the window (test_gpu_dt_accumulate.py, section 5)."""
    out = []
    for op, dt in TRIPLE:
        e = E(dt)
        for n in EDGE_NS:
            path = 1 if n == 1 else 2
            out.append(case(f"s3-{dt}-reg-{n}", 3, op, dt, n, ("vector", n, 1, 3, e), 1, "regular", n, path=path))
            blens, disps = cycle_blocks(n)
            out.append(case(f"s3-{dt}-tab-{n}", 3, op, dt, n, ("indexed", blens, disps, e), 1,
                            "regular" if n == 1 else "table", len(blens), path=path))
    return out


# ---- section 4: layout forms ---------------------------------------------------------

TRIPLE4 = (("MPI_SUM", "MPI_FLOAT"), ("MPI_BXOR", "MPI_INT16_T"), ("MPI_SUM", "MPI_C_DOUBLE_COMPLEX"))
PAD = {2: 2, 4: 4, 16: 8}        # keeps the element alignment, leaves the extents below off 16 bytes
TABLE_BLENS = [3, 1, 4, 1, 5, 2, 6, 2, 7]
TABLE_NRUNS = (2, 3, 4, 5, 8, 9)


def uneven(k, e):
    """k uneven blocks with gaps of one and two elements in turn."""
    blens, disps, at = TABLE_BLENS[:k], [], 0
    for j, b in enumerate(blens):
        disps.append(at)
        at += b + 1 + j % 2
    return ("indexed", blens, disps, e)


def _instances(per):
    return -(-(W + 1) // per)


def layouts(dt):
    """(tag, target recipe, target count, form, nruns) of section 4's layouts on
    the element `dt`.

    Which recipe reaches which regular form of build_dev_layout: a vector /
    hvector of one-run blocks sets t->rn (the compact form: `vector-b3`,
    `neg-stride`, `column`, `compact-vector`), a subarray or an hvector of
    such a vector adds t->rn2 (two levels), and a resized type copies either.
    An indexed / hindexed / indexed_block type always carries an explicit run
    list (t->rn == 0), which the `runs` loop finds regular when its blocks
    are uniform: `explicit-indexed`, `explicit-hindexed`, `explicit-iblock`.
    `one-run` is the explicit list with a single run (stride = len)."""
    e, s = E(dt), _esz(dt)
    pad = PAD[s]
    out = [
        ("one-run", ("resized", 0, 5 * s + pad, ("contig", 5, e)), 60, "regular", 1),
        ("vector-b3", ("resized", 0, 276 * s + pad, ("vector", 40, 3, 7, e)), 3, "regular", 40),
        ("neg-stride", ("resized", -4 * s, 52 * s, ("hvector", 15, 1, -3 * s, e)), 18, "regular", 15),
        ("column", ("resized", 0, s, ("vector", 40, 1, 7, e)), 7, "regular", 40),
        # two levels: rows of 9 (C) / 5 (Fortran) elements, and rows of one element
        ("sub3d-C-x1", ("subarray", [7, 9, 11], [5, 6, 9], [1, 2, 1], True, e), 1, "regular2", 30),
        ("sub3d-C-x3", ("subarray", [7, 9, 11], [5, 6, 9], [1, 2, 1], True, e), 3, "regular2", 30),
        ("sub3d-F-x1", ("subarray", [7, 9, 11], [5, 6, 9], [1, 2, 1], False, e), 1, "regular2", 54),
        ("sub3d-F-x3", ("subarray", [7, 9, 11], [5, 6, 9], [1, 2, 1], False, e), 3, "regular2", 54),
        ("sub3d-C-row1", ("subarray", [10, 31, 3], [9, 30, 1], [1, 0, 1], True, e), 1, "regular2", 270),
        ("sub3d-F-row1", ("subarray", [3, 31, 10], [1, 30, 9], [1, 1, 0], False, e), 2, "regular2", 270),
        ("hvec-of-vec-row1", ("hvector", 17, 1, 40 * s, ("vector", 16, 1, 2, e)), 1, "regular2", 272),
        ("hvec-of-vec-row3", ("hvector", 11, 1, 45 * s, ("vector", 8, 3, 5, e)), 1, "regular2", 88),
        # the same map from a compact form and from three explicit run lists
        ("compact-vector", ("vector", 130, 2, 5, e), 1, "regular", 130),
        ("explicit-indexed", ("indexed", [2] * 130, [5 * k for k in range(130)], e), 1, "regular", 130),
        ("explicit-hindexed", ("hindexed", [3] * 90, [7 * s * k for k in range(90)], e), 1, "regular", 90),
        ("explicit-iblock", ("iblock", 2, [5 * k for k in range(130)], e), 1, "regular", 130),
    ]
    for k in TABLE_NRUNS:
        out.append((f"table-{k}", uneven(k, e), _instances(sum(TABLE_BLENS[:k])), "table", k))
    out += [
        # displacements fall while packed offsets rise
        ("table-descending", ("indexed", [3, 1, 4, 1, 5], [20, 18, 12, 10, 0], e), 19, "table", 5),
        ("struct-gaps", ("struct", [2, 1, 3], [0, 3 * s, 5 * s], [e, e, e]), 45, "table", 3),
        ("struct-markers", ("struct", [1, 2, 3, 1, 1], [0, s, 5 * s, 9 * s, 12 * s], [LB, e, e, e, UB]), 45, "table", 3),
    ]
    return out


def _elements(trec, tcount, s):
    return build_oracle(trec).size * tcount // s


def section4():
    out = []
    for op, dt in TRIPLE4:
        for tag, trec, tcount, form, nruns in layouts(dt):
            out.append(case(f"s4-{tag}-{dt}", 4, op, dt, _elements(trec, tcount, _esz(dt)), trec, tcount, form, nruns))
    # misalignment from the layout alone: odd byte displacements, pointers on 16 bytes
    odd = {"MPI_FLOAT": ("hindexed", [2, 1, 3], [1, 15, 29], E("MPI_FLOAT")),
           "MPI_DOUBLE": ("hindexed", [2, 1, 3], [1, 23, 45], E("MPI_DOUBLE"))}
    for dt, trec in odd.items():
        out.append(case(f"s4-odd-disps-{dt}", 4, "MPI_SUM", dt, 300, trec, 50, "table", 3))
    # each source of ALIGNED = false on its own, then both pointers off by
    # alignof(T) = 8 (still the aligned form: complex doubles and the
    # double/double pair align to 8, not to their 16 bytes)
    for op, dt in (("MPI_SUM", "MPI_DOUBLE"), ("MPI_MAXLOC", "MPI_2DOUBLE_PRECISION")):
        for tag, trec, tcount, n, form, nruns, _ in four_forms(dt)[:2]:
            for mtag, mis in (("packed+1", (1, 0)), ("typed+1", (0, 1)), ("both+8", (8, 8))):
                out.append(case(f"s4-{mtag}-{dt}-{tag}", 4, op, dt, n, trec, tcount, form, nruns, mis=mis))
    # MPI_REPLACE (the unpack kernel) and MPI_NO_OP (no launch: path 0)
    for tag, trec, tcount, n, form, nruns, _ in four_forms("MPI_FLOAT")[:2]:
        out.append(case(f"s4-replace-{tag}", 4, "MPI_REPLACE", None, n, trec, tcount, form, nruns, edt="MPI_FLOAT"))
        out.append(case(f"s4-no-op-{tag}", 4, "MPI_NO_OP", None, n, trec, tcount, form, nruns, path=0, edt="MPI_FLOAT"))
    return out


def all_cases():
    return section1() + section2() + section3() + section4()


def run_args(c):
    """The arguments of test_gpu_accumulate_dev._run for a case."""
    data = operands(c) if c.data else None
    return (c.op, c.dt, E(c.edt), c.n, c.trec, c.tcount, c.path, c.mis_o, c.mis_t), {"data": data}
