"""The (op, element kind) kernel map (csrc/msx_op_kind.h) without a GPU.

tests/op_kind/op_kind_test.cpp, a host-only program that links msx_types.cpp,
walks the map through for_op / for_kind, the visitors every launcher uses:

* every predefined datatype under every builtin op the handle-level table
  allows (op_check_dtype) reaches an element type of TypeInfo::size bytes, and
  every accepted pair the exact C++ type of its kind (std::is_same against a
  list the program states itself, so int32_t for K_U32 or f16 for K_BF16 fails);
* the accepted (op, kind) set is the one the hand-written switches spelled out
  before the map replaced them, 124 pairs, and nothing else;
* the mask of the tree's per-op units drops exactly the 16-bit floats.
"""
import os
import subprocess

import pytest

import msx

DIR = os.path.join(msx.REPO_ROOT, "tests", "op_kind")

INTS = ["I8", "U8", "I16", "U16", "I32", "U32", "I64", "U64"]
FLOATS = ["F32", "F64"]
HALVES = ["F16", "BF16"]
COMPLEX = ["C32", "C64"]
LOCS = ["LOC_II", "LOC_FI", "LOC_SI", "LOC_DI", "LOC_FF", "LOC_DD"]
WANT = {}
for _op in ("MPI_MAX", "MPI_MIN"):
    WANT[_op] = INTS + FLOATS + HALVES
for _op in ("MPI_SUM", "MPI_PROD"):
    WANT[_op] = INTS + FLOATS + COMPLEX + HALVES
for _op in ("MPI_LAND", "MPI_LOR", "MPI_LXOR"):
    WANT[_op] = INTS + FLOATS + ["BOOL"]
for _op in ("MPI_BAND", "MPI_BOR", "MPI_BXOR"):
    WANT[_op] = INTS + ["BOOL"]
for _op in ("MPI_MAXLOC", "MPI_MINLOC"):
    WANT[_op] = LOCS
# op indices with no kernel of their own, and one past the last
NO_KERNEL = ["MPI_OP_NULL", "MPI_REPLACE", "MPI_NO_OP", "MSX_SUM_WIDE", "O_COUNT"]


@pytest.fixture(scope="module")
def report():
    r = subprocess.run(["make", "-C", DIR, "build/op_kind_test"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run([os.path.join(DIR, "build", "op_kind_test")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = {"OP": {}, "TREE": {}}
    for line in r.stdout.splitlines():
        p = line.split()
        assert p[0] != "FAIL", line
        if p[0] in ("OP", "TREE"):
            out[p[0]][p[1]] = p[2:]
        else:
            out[p[0]] = int(p[1])
    return out


def test_every_legal_pair_reaches_an_element_of_the_tables_size(report):
    assert report["FAILS"] == 0
    # the whole table was walked: 56 predefined reducible datatypes today, and
    # never fewer legal pairs than the 22-datatype subset's 125
    assert report["TYPES"] >= 56
    assert report["LEGAL"] >= 125


def test_accepted_pairs_are_exactly_the_switches_set(report):
    got = report["OP"]
    assert sorted(got) == sorted(list(WANT) + NO_KERNEL)
    for op, kinds in WANT.items():
        assert sorted(got[op]) == sorted(kinds), op
    for op in NO_KERNEL:
        assert got[op] == [], op
    by_class = {op: len(k) for op, k in got.items() if k}
    assert by_class == {"MPI_MAX": 12, "MPI_MIN": 12, "MPI_SUM": 14, "MPI_PROD": 14,
                        "MPI_LAND": 11, "MPI_LOR": 11, "MPI_LXOR": 11,
                        "MPI_BAND": 9, "MPI_BOR": 9, "MPI_BXOR": 9, "MPI_MAXLOC": 6, "MPI_MINLOC": 6}
    assert sum(by_class.values()) == 124
    # K_NONE and K_COUNT have no kernel under any op
    assert not any(k in ("NONE", "COUNT") for kinds in got.values() for k in kinds)


def test_tree_mask_excludes_exactly_the_16_bit_floats(report):
    for op, kinds in report["OP"].items():
        assert report["TREE"][op] == [k for k in kinds if k not in HALVES], op
    assert any(set(HALVES) <= set(kinds) for kinds in report["OP"].values())
