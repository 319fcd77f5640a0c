"""The combine plan of the user-op collectives (userop_plan, msx_schedule.cpp),
which the host path and the device path both execute.

ORDER: p host processes run every user-op collective with the non-associative,
non-commutative twin 3 * in - inout on uint32 (exact under wrap) and each rank
compares its bytes with tests/_userop_ref.py, an independent numpy simulation
of all p ranks of the reference's schedules.  The worker also counts the calls
of the user function: the host path evaluates the asking rank's value only
(DESIGN.md section 4).

PLAN: msx_schedule_userop_plan evaluated symbolically equals the tree
msx_schedule_devop_tree reports wherever that exists, and every plan reads each
block exactly once.  No GPU needed."""
import ctypes
import os
import socket
import subprocess
import sys
import textwrap

import pytest

import msx
from _devop_tree_ref import devop_tree_spec, tree_value

C = msx.C
REPO = msx.REPO_ROOT

ORDER_WORKER = r'''
import ctypes, os, sys
sys.path.insert(0, os.path.join(REPO, "microsoft-mpi_amd")); sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np
import msx
import _userop_ref as ref
from _devop_tree_ref import nc
C = msx.C
L = msx.init(errors_return=True)
r_, s_ = ctypes.c_int(), ctypes.c_int()
L.MPI_Comm_rank(C.MPI_COMM_WORLD, ctypes.byref(r_)); L.MPI_Comm_size(C.MPI_COMM_WORLD, ctypes.byref(s_))
rank, p = r_.value, s_.value
W, U, N = C.MPI_COMM_WORLD, C.MPI_UNSIGNED, 5
PAIRWISE = os.environ.get("MPICH_DEFAULT_REDSCAT_COMMUTATIVE_LONG_MSG") == "0"
UF = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int))
calls = [0]
def twin(a, b, n, dt):          # inout = 3 * in - inout
    calls[0] += 1
    x = np.ctypeslib.as_array((ctypes.c_uint32 * n[0]).from_address(a))
    y = np.ctypeslib.as_array((ctypes.c_uint32 * n[0]).from_address(b))
    y[:] = nc(x, y)
fn = UF(twin)
L.MPI_Iscan.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                        ctypes.c_void_p]
def x_of(r, n, seed):
    return np.random.default_rng([seed, r]).integers(0, 2**32, n, dtype=np.uint32)
SENT = np.uint32(0xA5A5A5A5)
fails, over = [], []
def check(tag, bound, got, exp):
    """every byte of recvbuf (exp None: the sentinel is still there) and the calls of the user function"""
    if exp is None:
        exp = np.full(got.size, SENT)
    print("CALLS", tag, calls[0], bound, flush=True)
    if got.tobytes() != exp.tobytes():
        fails.append(tag)
    if calls[0] > bound:
        over.append((tag, calls[0], bound))
    calls[0] = 0
for commute in (0, 1):
    op = ctypes.c_int()
    assert L.MPI_Op_create(fn, commute, ctypes.byref(op)) == 0
    xs = [x_of(r, N, 1 + commute) for r in range(p)]
    got = np.full(N, SENT)
    assert L.MPI_Allreduce(xs[rank].ctypes.data, got.ctypes.data, N, U, op.value, W) == 0, msx.last_error()
    check(f"allreduce commute={commute}", p - 1, got, ref.allreduce(xs, nc, commute)[rank])
    for root in (0, p - 1):
        got = np.full(N, SENT)
        assert L.MPI_Reduce(xs[rank].ctypes.data, got.ctypes.data, N, U, op.value, root, W) == 0, msx.last_error()
        check(f"reduce root={root} commute={commute}", p - 1 if rank == root else 0, got,
              ref.reduce(xs, nc, commute, root) if rank == root else None)
    xs = [x_of(r, p * N, 3 + commute) for r in range(p)]
    got = np.full(N, SENT)
    assert L.MPI_Reduce_scatter_block(xs[rank].ctypes.data, got.ctypes.data, N, U, op.value, W) == 0, msx.last_error()
    check(f"reduce_scatter_block commute={commute}", p - 1, got,
          ref.reduce_scatter(xs, nc, commute, PAIRWISE)[rank][rank * N:(rank + 1) * N])
    # MPI_Reduce_scatter: blocks of 1 .. p elements, rank p // 2 receives nothing
    counts = [0 if r == p // 2 else r + 1 for r in range(p)]
    disp = np.concatenate(([0], np.cumsum(counts)))
    xs = [x_of(r, int(disp[p]), 5 + commute) for r in range(p)]
    got = np.full(p + 1, SENT)
    rcounts = (ctypes.c_int * p)(*counts)
    assert L.MPI_Reduce_scatter(xs[rank].ctypes.data, got.ctypes.data, rcounts, U, op.value, W) == 0, msx.last_error()
    exp = np.full(p + 1, SENT)
    exp[:counts[rank]] = ref.reduce_scatter(xs, nc, commute, PAIRWISE)[rank][disp[rank]:disp[rank + 1]]
    check(f"reduce_scatter commute={commute}", p - 1, got, exp)
    xs = [x_of(r, N, 7 + commute) for r in range(p)]
    for name, f, excl in (("scan", L.MPI_Scan, False), ("exscan", L.MPI_Exscan, True)):
        got = np.full(N, SENT)
        assert f(xs[rank].ctypes.data, got.ctypes.data, N, U, op.value, W) == 0, msx.last_error()
        check(f"{name} commute={commute}", 2 * (p - 1), got, ref.scan(xs, nc, commute, excl)[rank])
    got, req = np.full(N, SENT), ctypes.c_int()
    assert L.MPI_Iscan(xs[rank].ctypes.data, got.ctypes.data, N, U, op.value, W, ctypes.byref(req)) == 0
    assert L.MPI_Wait(ctypes.byref(req), ctypes.c_void_p(1)) == 0 and req.value == C.MPI_REQUEST_NULL
    check(f"iscan commute={commute}", 2 * (p - 1), got, ref.scan(xs, nc, commute, False)[rank])
    assert L.MPI_Op_free(ctypes.byref(op)) == 0
print("RESULT", rank, p, len(fails), len(over), fails, over, flush=True)
assert L.MPI_Finalize() == 0
'''


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _run_order(p, extra_env):
    port = _free_port()
    procs = []
    for r in range(p):
        env = dict(os.environ)
        env.update({"MSX_SIZE": str(p), "MSX_RANK": str(r), "MSX_BOOTSTRAP_PORT": str(port),
                    "MSX_BOOTSTRAP_ADDR": "127.0.0.1"})
        env.update(extra_env)
        procs.append(subprocess.Popen([sys.executable, "-c", f"REPO={REPO!r}\n" + textwrap.dedent(ORDER_WORKER)],
                                      stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env))
    outs = []
    for pr in procs:
        try:
            o, e = pr.communicate(timeout=240)
        except subprocess.TimeoutExpired:
            pr.kill()
            o, e = pr.communicate()
        outs.append((pr.returncode, o, e))
    seen, bytes_differ, calls_over = set(), [], []
    for rc, o, e in outs:
        assert rc == 0, (o + e)[-3000:]
        line = [l for l in o.splitlines() if l.startswith("RESULT")][0].split(" ", 5)
        assert int(line[2]) == p, o
        if int(line[3]):
            bytes_differ.append(line[1] + ": " + line[5])
        if int(line[4]):
            calls_over.append(line[1] + ": " + line[5])
        seen.add(int(line[1]))
    assert seen == set(range(p))
    assert not bytes_differ, "bytes differ from the reference order, by rank: " + str(bytes_differ)
    assert not calls_over, "more calls of the user function than the plan has steps, by rank: " + str(calls_over)


# p = 3, 5, 6, 7, 9: folds, absent binomial leaves, partial scan steps
@pytest.mark.parametrize("p", [2, 3, 4, 5, 6, 7, 8, 9])
def test_host_path_is_the_reference_order(p):
    _run_order(p, {})


# the commutative reduce_scatter's pairwise chain, which N = 5 elements reach
# only with the long-message gate moved to 0 bytes
@pytest.mark.parametrize("p", [3, 8])
def test_host_path_is_the_reference_order_pairwise_reduce_scatter(p):
    _run_order(p, {"MPICH_DEFAULT_REDSCAT_COMMUTATIVE_LONG_MSG": "0"})


# ---- the plan itself ---------------------------------------------------------
ALLREDUCE, REDUCE, REDUCE_SCATTER, SCAN = 0, 1, 2, 3
SMALL, LARGE = 100, 1 << 20          # x 4 bytes: below / above the reduce_scatter gate of 512 KiB


def userop_plan(L, which, p, n, commutative, exclusive, total_count, type_size=4):
    """msx_schedule_userop_plan -> (rc, [(in, io), ...], result)"""
    cap = 2 * p
    steps = (ctypes.c_int * (2 * cap))()
    ns, res = ctypes.c_int(-7), ctypes.c_int(-7)
    rc = L.msx_schedule_userop_plan(which, p, n, commutative, exclusive, total_count, type_size, steps, cap,
                                    ctypes.byref(ns), ctypes.byref(res))
    return rc, [(steps[2 * k], steps[2 * k + 1]) for k in range(ns.value)] if rc == 0 else [], res.value


def _cases(p):
    for commutative in (0, 1):
        for n in range(p):
            yield ALLREDUCE, n, commutative, 0, p
            yield REDUCE, n, commutative, 0, p
            yield REDUCE_SCATTER, n, commutative, 0, SMALL
            yield REDUCE_SCATTER, n, commutative, 0, LARGE
            yield SCAN, n, commutative, 0, p
            yield SCAN, n, commutative, 1, p


def _leaves(expr):
    return sorted(int(t) for t in expr.replace("f(", "").replace(")", "").replace("x", "").split(","))


def _check_plan(L, p, which, n, commutative, exclusive, count):
    """-> the symbolic value of the plan, after the properties every plan has"""
    tag = (which, p, n, commutative, exclusive, count)
    rc, steps, result = userop_plan(L, which, p, n, commutative, exclusive, count)
    assert rc == 0, tag
    if which == SCAN:
        assert len(steps) <= 2 * (p - 1), tag
    else:
        assert len(steps) == p - 1, tag
    v = [f"x{r}" for r in range(p)]
    consumed = [False] * p
    for a, b in steps:
        assert 0 <= a < p and 0 <= b < p and a != b, tag
        assert not consumed[a] and not consumed[b], tag        # a block is an operand as `in` once, and is gone
        consumed[a] = True
        v[b] = f"f({v[a]},{v[b]})"
    if which == SCAN:
        # ranks above n are not part of n's prefix: their blocks are never touched
        untouched = [r for r in range(p) if not consumed[r] and v[r] == f"x{r}"]
        live = [r for r in range(p) if not consumed[r] and r not in untouched]
        if exclusive and n == 0:
            assert result == -1 and not steps, tag
            return None
        if not live:                                       # the value is one untouched block
            assert result in untouched and (result == n) != bool(exclusive), tag
        else:
            assert live == [result], tag
        assert _leaves(v[result]) == list(range(n + (0 if exclusive else 1))), tag
    else:
        # every block was consumed but one: the result, never `in` after its last write
        assert [r for r in range(p) if not consumed[r]] == [result], tag
        assert _leaves(v[result]) == list(range(p)), tag
    return v[result]


def test_plan_is_the_tree_spec_and_reads_each_block_once(msxlib):
    L = msxlib

    def g(a, b):
        return f"f({a},{b})"

    matched = 0
    for p in range(2, 32):
        for which, n, commutative, exclusive, count in _cases(p):
            value = _check_plan(L, p, which, n, commutative, exclusive, count)
            if which == SCAN:
                continue
            rc, src, P, pm, nl, ch, il = devop_tree_spec(L, which, p, n, commutative, count, 4)
            if rc != 0:
                continue
            want = tree_value([f"x{r}" if r >= 0 else None for r in src], P, pm, nl, ch, il, g)
            assert value == want, (which, p, n, commutative, count)
            matched += 1
    assert matched > 2000


@pytest.mark.parametrize("p", [32, 33, 64])
def test_plans_beyond_the_kernels_leaves(msxlib, p):
    for which, n, commutative, exclusive, count in _cases(p):
        _check_plan(msxlib, p, which, n, commutative, exclusive, count)


def test_scan_plan_values(msxlib):
    """the recursive-doubling prefixes of tests/test_collectives_cpu.py's scan test, from the plan"""
    L = msxlib

    def value(n, exclusive):
        return _check_plan(L, 4, SCAN, n, 0, exclusive, 4)

    assert [value(n, 0) for n in range(4)] == ["x0", "f(x0,x1)", "f(f(x0,x1),x2)", "f(f(x0,x1),f(x2,x3))"]
    assert [value(n, 1) for n in range(4)] == [None, "x0", "f(x0,x1)", "f(f(x0,x1),x2)"]


def test_plan_argument_checks(msxlib):
    L = msxlib
    E = C.MPI_ERR_ARG
    assert userop_plan(L, 4, 4, 0, 1, 0, 4)[0] == E and userop_plan(L, -1, 4, 0, 1, 0, 4)[0] == E
    assert userop_plan(L, 0, 0, 0, 1, 0, 4)[0] == E
    assert userop_plan(L, 0, 4, 4, 1, 0, 4)[0] == E and userop_plan(L, 0, 4, -1, 1, 0, 4)[0] == E
    assert userop_plan(L, 0, 4, 0, 1, 0, -1)[0] == E and userop_plan(L, 0, 4, 0, 1, 0, 4, -1)[0] == E
    ns, res = ctypes.c_int(), ctypes.c_int()
    steps = (ctypes.c_int * 16)()
    assert L.msx_schedule_userop_plan(0, 4, 0, 1, 0, 4, 4, None, 8, ctypes.byref(ns), ctypes.byref(res)) == E
    assert L.msx_schedule_userop_plan(0, 4, 0, 1, 0, 4, 4, steps, 8, None, ctypes.byref(res)) == E
    assert L.msx_schedule_userop_plan(0, 4, 0, 1, 0, 4, 4, steps, 8, ctypes.byref(ns), None) == E
    # a buffer too small for the steps: nothing written beyond cap, the count still reported
    assert L.msx_schedule_userop_plan(0, 4, 0, 1, 0, 4, 4, steps, 2, ctypes.byref(ns), ctypes.byref(res)) == E
    assert ns.value == 3
    # one rank: no step, the rank's own block
    assert userop_plan(L, 0, 1, 0, 1, 0, 4) == (0, [], 0)
    assert userop_plan(L, 3, 1, 0, 1, 1, 4) == (0, [], -1)
