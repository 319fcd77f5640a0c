"""CPU, no GPU: the case table of tests/test_gpu_dt_accumulate.py
(tests/_dt_acc_cases.py) is what it claims to be.

msx_accumulate_plan is a pure function of its arguments, so every case's path
and granule are checked here; the oracle's type maps show that every target
map is disjoint, that the origin covers whole target instances, and that each
layout has the form (regular, two-level regular, run table) and the number of
runs its case states.  The counts are pinned, so a case cannot be dropped
quietly."""
import ctypes
from collections import Counter

import numpy as np
import pytest

import msx
import _dt_acc_cases as T
from _cases import KIND, OPS, h
from test_dtype_cpu import build_lib, build_oracle, free_all
from test_gpu_accumulate_dev import PAIR_TYPES, W, _data_bytes, _pairs
from test_gpu_batch_local import _esz

C = msx.C
i64, c_int = ctypes.c_int64, ctypes.c_int


@pytest.fixture(scope="module")
def L():
    return msx.init(errors_return=True)


@pytest.fixture(scope="module")
def cases():
    return T.all_cases()


def test_ids_are_unique(cases):
    assert len({c.id for c in cases}) == len(cases)


def test_every_case_plans_its_path_with_the_element_as_granule(L, cases):
    for c in cases:
        keep = []
        th = build_lib(L, c.trec, keep)
        x = c_int(th)
        assert L.MPI_Type_commit(ctypes.byref(x)) == 0
        n, path, gran = i64(-7), c_int(-7), c_int(-7)
        rc = L.msx_accumulate_plan(c.n, h(c.edt), c.tcount, th, h(c.op), ctypes.byref(n), ctypes.byref(path),
                                   ctypes.byref(gran))
        assert rc == 0, (c.id, msx.last_error())
        assert (n.value, path.value) == (c.n, c.path), c.id
        if c.op != "MPI_NO_OP":
            assert gran.value == _esz(c.edt), c.id
        free_all(L, keep)
    assert Counter(c.path for c in cases if c.op == "MPI_NO_OP") == {0: 2}
    # path 1 only where section 3 says why: the one-element targets
    assert {c.id for c in cases if c.path == 1} == {c.id for c in T.section3() if c.n == 1}


def test_target_maps_are_disjoint_and_whole_instances_are_covered(cases):
    seen = {}
    for c in cases:
        key = repr((c.trec, c.tcount))
        if key not in seen:
            t = build_oracle(c.trec)
            tb = _data_bytes(t, c.tcount, 0)
            seen[key] = (t.size * c.tcount, np.unique(tb).size == tb.size, T.layout_of(t))
        size, disjoint, layout = seen[key]
        esz = _esz(c.edt)
        assert disjoint, c.id
        assert c.n * esz == size, c.id                                   # whole instances
        assert size // esz <= 1000, c.id
        assert layout == (c.form, c.nruns), (c.id, layout)
        assert c.mis_o < 16 and c.mis_t < 16


def test_section_1_holds_every_pair_in_every_form_it_has():
    pairs = _pairs()
    s1 = T.section1()
    one_byte = [p for p in pairs if _esz(p[1]) == 1]
    assert one_byte and len(s1) == 4 * len(pairs) - 2 * len(one_byte)
    assert {_esz(c.dt) for c in s1} == {1, 2, 4, 8, 16}
    assert {c.op for c in s1} == set(OPS)
    assert not {c.dt for c in s1} & set(PAIR_TYPES)
    for p in pairs:
        mine = [c for c in s1 if (c.op, c.dt) == p]
        want = {("regular", 0, 0), ("table", 0, 0)}
        if _esz(p[1]) > 1:
            want |= {("regular", 1, 3), ("table", 1, 3)}
        assert {(c.form, c.mis_o, c.mis_t) for c in mine} == want and len(mine) == len(want), p
        assert all(c.n > W and c.n - W <= 16 for c in mine)              # a second tile with few live lanes
    # the 2-byte and wider kinds the other sweeps never run element-typed
    kinds = {(c.op, KIND.get(c.dt, c.dt)) for c in s1}
    for op in ("MPI_BAND", "MPI_BOR", "MPI_BXOR"):
        assert {(op, k) for k in ("i1", "u1", "i2", "u2", "i4", "u4", "i8", "u8")} <= kinds
    for k in ("ii", "ff", "dd"):
        assert ("MPI_MAXLOC", k) in kinds and ("MPI_MINLOC", k) in kinds


def test_section_2_leads_with_the_full_ordered_cross_product():
    s2 = T.section2()
    assert len(s2) == 4 * len(T.DIRECTED) and len(T.DIRECTED) == 8 + 8 + 4
    for op, dt, key in T.DIRECTED:
        vals = T.OPERANDS[key](dt)
        if key != "loc":
            assert len(vals) == 15
        raw = [vals[k:k + 1].tobytes() for k in range(len(vals))]
        o, t = T.cross(vals)
        got = {(o[k:k + 1].tobytes(), t[k:k + 1].tobytes()) for k in range(o.size)}
        assert got == {(a, b) for a in raw for b in raw}
        esz = _esz(dt)
        for c in T.directed_cases((op, dt, key)):
            ob, tb = T.operands(c)
            assert ob.size == tb.size == c.n * esz
            assert ob[:o.size * esz].tobytes() == o.tobytes() and tb[:o.size * esz].tobytes() == t.tobytes()
    # what makes the order visible: two NaNs that differ in sign and payload, and both zeros
    for dt in ("MPI_FLOAT", "MPI_DOUBLE"):
        v = T.OPERANDS["float"](dt)
        nans = v[np.isnan(v)]
        assert len({x.tobytes() for x in nans}) == 3 and len({bool(np.signbit(x)) for x in nans}) == 2
        assert {bool(np.signbit(x)) for x in v[v == 0]} == {False, True}
    for dt in T.R.TYPES:
        w = T.R.W[dt](T.OPERANDS["half"](dt))
        assert np.isnan(w).sum() >= 2 and {bool(np.signbit(x)) for x in w[w == 0]} == {False, True}
        assert np.isposinf(w).any() and np.isneginf(w).any()
    for dt in ("MPI_2REAL", "MPI_2INT"):
        v = T.OPERANDS["loc"](dt)
        # equal values at differing locations; the cross product above holds both orders
        assert any(a["v"] == b["v"] and a["l"] < b["l"] for a in v for b in v)
    assert np.isnan(T.OPERANDS["loc"]("MPI_2REAL")["v"]).sum() == 2


def test_sections_3_and_4_hold_the_counts_and_run_numbers_listed():
    s3 = T.section3()
    assert len(s3) == 3 * 2 * len(T.EDGE_NS)
    assert T.EDGE_NS == (1, 63, 64, 65, W - 1, W, W + 1, 3 * W + 5)
    assert {_esz(dt) for _, dt in T.TRIPLE} == {2, 4, 16}
    for _, dt in T.TRIPLE:
        assert [c.n for c in s3 if c.dt == dt and "-reg-" in c.id] == list(T.EDGE_NS)
        assert [c.n for c in s3 if c.dt == dt and "-tab-" in c.id] == list(T.EDGE_NS)
    for n in T.EDGE_NS:
        blens, disps = T.cycle_blocks(n)
        assert sum(blens) == n and blens[:-1] == [(1, 2, 3)[k % 3] for k in range(len(blens) - 1)]
        assert all(d1 == d0 + b0 + 1 for d0, b0, d1 in zip(disps, blens, disps[1:]))
    s4 = T.section4()
    by = lambda tag: [c for c in s4 if c.id.startswith("s4-" + tag)]
    for k in T.TABLE_NRUNS:
        assert [(c.form, c.nruns) for c in by(f"table-{k}-")] == [("table", k)] * 3
    assert T.TABLE_NRUNS == (2, 3, 4, 5, 8, 9)
    assert [(c.form, c.nruns, c.tcount) for c in by("one-run")] == [("regular", 1, 60)] * 3
    for tag in ("compact-vector", "explicit-indexed", "explicit-hindexed", "explicit-iblock", "vector-b3",
                "neg-stride", "column"):
        assert [c.form for c in by(tag)] == ["regular"] * 3, tag
    assert len([c for c in s4 if c.form == "regular2"]) == 3 * 8
    assert {c.tcount for c in by("sub3d")} == {1, 2, 3}
    # every layout of the list on all three element sizes, spanning more than a tile
    per = len(T.layouts("MPI_FLOAT"))
    assert per == 25
    for _, dt in T.TRIPLE4:
        mine = [c for c in s4 if c.dt == dt and c.id.endswith("-" + dt) and "odd-disps" not in c.id]
        assert len(mine) == per and all(c.n > W for c in mine), dt
    # extents that are no multiple of 16 where the issue asks for one
    for c in by("one-run") + by("vector-b3"):
        assert build_oracle(c.trec).extent % 16 != 0 and build_oracle(c.trec).extent % min(_esz(c.dt), 8) == 0
    # the unaligned form from the layout alone, and from each pointer alone
    assert [(c.dt, c.mis_o, c.mis_t) for c in by("odd-disps")] == [("MPI_FLOAT", 0, 0), ("MPI_DOUBLE", 0, 0)]
    for c in by("odd-disps"):
        assert any(d % _esz(c.dt) for d, _ in build_oracle(c.trec).typemap)
    alone = Counter((c.dt, c.form, c.mis_o, c.mis_t) for c in by("packed+1") + by("typed+1") + by("both+8"))
    assert alone == {(dt, f, *m): 1 for dt in ("MPI_DOUBLE", "MPI_2DOUBLE_PRECISION") for f in ("regular", "table")
                     for m in ((1, 0), (0, 1), (8, 8))}
    assert Counter((c.op, c.form) for c in s4 if c.dt is None) == {
        (op, f): 1 for op in ("MPI_REPLACE", "MPI_NO_OP") for f in ("regular", "table")}
