"""The fused tree form of device user ops (msx_op_create_device_tree): handles,
the hook's validation and refusals with ctypes callbacks as the functions, the
spec introspection, and the ORDER -- p host processes run the user-op
collectives with a host twin of 3 * in - inout and every rank compares its
bytes with a numpy evaluation (tests/_devop_tree_ref.py, written from the
header's definition of the value) of the spec msx_schedule_devop_tree reports
for the call, so the spec the device path hands to a tree function is pinned to
the pairwise path that defines it.  No GPU needed."""
import ctypes
import os
import socket
import subprocess
import sys
import textwrap

import pytest

import msx
from _devop_tree_ref import devop_tree_spec

C = msx.C
REPO = msx.REPO_ROOT

DF = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int,
                      ctypes.c_void_p, ctypes.c_void_p)
# MSX_Device_tree_function
TF = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, ctypes.c_int, ctypes.c_int,
                      ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p)
UF = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int),
                      ctypes.POINTER(ctypes.c_int))


def _tree_op(L, fn, tree_fn, commute=0, state=None):
    op = ctypes.c_int(0)
    assert L.msx_op_create_device_tree(fn, tree_fn, commute, state, ctypes.byref(op)) == 0, msx.last_error()
    return op


def test_registration_rules(msxlib):
    L = msxlib
    fn, tf = DF(lambda *a: 0), TF(lambda *a: 0)
    op = ctypes.c_int(0)
    assert L.msx_op_create_device_tree(None, tf, 1, None, ctypes.byref(op)) == C.MPI_ERR_ARG
    assert L.msx_op_create_device_tree(fn, tf, 1, None, None) == C.MPI_ERR_ARG
    c = ctypes.c_int(-1)
    for commute in (0, 1):
        op = _tree_op(L, fn, tf, commute)
        assert (op.value & 0xFC000000) == 0x98000000          # the pool of MPI_Op_create
        assert L.MPI_Op_commutative(op.value, ctypes.byref(c)) == 0 and c.value == commute
        assert L.msx_op_is_device(op.value) == 1 and L.msx_op_has_device_tree(op.value) == 1
        old = op.value
        assert L.MPI_Op_free(ctypes.byref(op)) == 0 and op.value == C.MPI_OP_NULL
        assert L.msx_op_has_device_tree(old) == -1


def test_has_device_tree_tells_the_kinds_apart(msxlib):
    L = msxlib
    fn, tf = DF(lambda *a: 0), TF(lambda *a: 0)
    with_tree, without = _tree_op(L, fn, tf), _tree_op(L, fn, None)
    plain = ctypes.c_int(0)
    assert L.msx_op_create_device(fn, 1, None, ctypes.byref(plain)) == 0
    hf = UF(lambda a, b, n, d: None)
    hop = ctypes.c_int(0)
    assert L.MPI_Op_create(hf, 1, ctypes.byref(hop)) == 0
    assert L.msx_op_has_device_tree(with_tree.value) == 1
    # a NULL tree function: exactly msx_op_create_device's op
    assert L.msx_op_has_device_tree(without.value) == 0 and L.msx_op_is_device(without.value) == 1
    assert L.msx_op_has_device_tree(plain.value) == 0
    assert L.msx_op_has_device_tree(hop.value) == 0
    assert L.msx_op_has_device_tree(C.MPI_SUM) == 0
    assert L.msx_op_has_device_tree(C.MPI_OP_NULL) == -1
    assert L.msx_op_has_device_tree(0x98000000 | 0x3ffff) == -1
    for o in (with_tree, without, plain, hop):
        assert L.MPI_Op_free(ctypes.byref(o)) == 0
    assert C.MSX_TREE_DECLINED == -1


def test_hook_checks_its_arguments_before_the_function_is_entered(msxlib):
    L = msxlib
    entered = []

    def tree(*a):
        entered.append(a)
        return C.MSX_TREE_DECLINED

    def pair(*a):
        entered.append(a)
        return 0

    fn, tf = DF(pair), TF(tree)
    op, without = _tree_op(L, fn, tf), _tree_op(L, fn, None)
    srcs = (ctypes.c_void_p * 32)(*([0x1000] * 32))      # never dereferenced by the library
    out, U = ctypes.c_void_p(0x2000), C.MPI_UNSIGNED

    def hook(P, pm, nl, chain, il, count=8, srcs=srcs, out=out, o=None):
        return L.msx_reduce_tree_user_dev(srcs, P, pm, nl, chain, il, out, count, U, op.value if o is None else o, None)

    A = C.MPI_ERR_ARG
    assert hook(4, 0, 0, 0, 0, srcs=None) == A
    assert hook(4, 0, 0, 0, 0, out=None) == A
    for P in (0, 3, 5, 6, 12, 32, -1):
        assert hook(P, 0, 0, 0, 0) == A, P
    for P in (0, 1, 17, -2):
        assert hook(P, 0, 0, 1, 0) == A, P
    assert hook(4, 0, 5, 0, 0) == A and hook(4, 0, -1, 0, 0) == A
    assert hook(4, 0b10000, 0, 0, 0) == A            # a pair at or above P
    assert hook(4, 0b0100, 2, 0, 0) == A             # a pair at or above nleaves
    assert hook(8, 0b1000, 3, 0, 0) == A
    assert hook(4, 0b0001, 0, 1, 0) == A             # a chain has no pairs
    assert hook(4, 0, 4, 1, 0) == A                  # and no nleaves
    assert hook(4, 0, 0, 0, 2) == A and hook(4, 0, 0, 0, -1) == A
    assert hook(4, 0, 0, 0, 0, count=-1) == C.MPI_ERR_COUNT
    # an op without a tree function, whatever it is: never the pairwise path
    assert hook(4, 0, 0, 0, 0, o=without.value) == C.MPI_ERR_OP
    assert hook(4, 0, 0, 0, 0, o=C.MPI_SUM) == C.MPI_ERR_OP
    assert hook(4, 0, 0, 0, 0, o=C.MPI_OP_NULL) == C.MPI_ERR_OP
    assert hook(4, 0, 0, 0, 0, count=0) == 0         # nothing to do, no call
    assert not entered
    # a valid call: without a GPU MPI_ERR_OTHER and the function is never
    # entered; with one the function's own answer comes back
    for spec in ((4, 0b0011, 0, 0, 1), (8, 0, 5, 0, 0), (16, 0, 0, 1, 1), (1, 0, 0, 0, 0), (2, 0, 0, 1, 0)):
        rc = hook(*spec)
        if L.msx_device_count() == 0:
            assert rc == C.MPI_ERR_OTHER and not entered
        else:
            assert rc == C.MSX_TREE_DECLINED and len(entered) == 1
            got = entered.pop()
            assert got[1:6] == spec and got[7] == 8 and got[8] == U
    assert L.MPI_Op_free(ctypes.byref(op)) == 0 and L.MPI_Op_free(ctypes.byref(without)) == 0


def test_spec_introspection_shapes_and_limits(msxlib):
    L = msxlib
    E = C.MPI_ERR_ARG
    # beyond 16 leaves the collectives keep the pairwise evaluation
    assert devop_tree_spec(L, 0, 31, 0, 1, 31, 4)[0] == 0 and devop_tree_spec(L, 0, 32, 0, 1, 32, 4)[0] == E
    assert devop_tree_spec(L, 1, 16, 3, 1, 16, 4)[0] == 0 and devop_tree_spec(L, 1, 17, 3, 1, 17, 4)[0] == E
    small, large = 100, 1 << 20                      # the gate: total bytes below / at 512 KiB
    assert devop_tree_spec(L, 2, 31, 5, 1, small, 4)[0] == 0
    assert devop_tree_spec(L, 2, 16, 5, 1, large, 4)[0] == 0 and devop_tree_spec(L, 2, 17, 5, 1, large, 4)[0] == E
    assert devop_tree_spec(L, 2, 31, 5, 0, large, 4)[0] == 0      # non-commutative: the allreduce tree
    assert devop_tree_spec(L, 3, 4, 0, 1, 4, 4)[0] == E and devop_tree_spec(L, 0, 4, 4, 1, 4, 4)[0] == E
    assert devop_tree_spec(L, 0, 1, 0, 1, 4, 4)[0] == E
    for p in range(2, 17):
        for commutative in (0, 1):
            for which, count in ((0, p), (1, p), (2, small), (2, large)):
                for n in range(p):
                    rc, src, P, pm, nl, ch, il = devop_tree_spec(L, which, p, n, commutative, count, 4)
                    assert rc == 0
                    used = [r for r in src if r >= 0]
                    # every rank's contribution is read exactly once
                    assert sorted(used) == list(range(p)), (which, p, n, commutative, src)
                    if ch:
                        assert which == 2 and commutative and count == large and P == p and pm == 0 and nl == 0
                        assert src[:p] == [(n - k) % p for k in range(p)] and il == 0
                        continue
                    assert P & (P - 1) == 0 and P <= 16 and pm >> (nl or P) == 0
                    for k in range(P):
                        assert (src[2 * k] >= 0) == (k < (nl or P)) and (src[2 * k + 1] >= 0) == bool(pm >> k & 1)
                    assert il == (0 if commutative else 1)
                    if which == 1:
                        assert nl == p and pm == 0 and P >= p and P < 2 * p
                        assert [src[2 * k] for k in range(p)] == [(k + (n if commutative else 0)) % p for k in range(p)]
                    else:
                        assert nl == 0 and P <= p < 2 * P and bin(pm).count("1") == p - P


ORDER_WORKER = r'''
import ctypes, os, sys
sys.path.insert(0, os.path.join(REPO, "microsoft-mpi_amd")); sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np
import msx
from _devop_tree_ref import nc, spec_value
C = msx.C
L = msx.init(errors_return=True)
r_, s_ = ctypes.c_int(), ctypes.c_int()
L.MPI_Comm_rank(C.MPI_COMM_WORLD, ctypes.byref(r_)); L.MPI_Comm_size(C.MPI_COMM_WORLD, ctypes.byref(s_))
rank, p = r_.value, s_.value
W, U, N = C.MPI_COMM_WORLD, C.MPI_UNSIGNED, 5
UF = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int))
def twin(a, b, n, dt):          # the host twin of Nc<uint32_t>: inout = 3 * in - inout
    x = np.ctypeslib.as_array((ctypes.c_uint32 * n[0]).from_address(a))
    y = np.ctypeslib.as_array((ctypes.c_uint32 * n[0]).from_address(b))
    y[:] = nc(x, y)
fn = UF(twin)
def x_of(r, n, seed):
    return np.random.default_rng([seed, r]).integers(0, 2**32, n, dtype=np.uint32)
fails = []
def same(tag, got, exp):
    if got.tobytes() != exp.tobytes():
        fails.append(tag)
SENT = np.uint32(0xA5A5A5A5)
for commute in (0, 1):
    op = ctypes.c_int()
    assert L.MPI_Op_create(fn, commute, ctypes.byref(op)) == 0
    xs = [x_of(r, N, 1 + commute) for r in range(p)]
    got = np.full(N, SENT)
    assert L.MPI_Allreduce(xs[rank].ctypes.data, got.ctypes.data, N, U, op.value, W) == 0, msx.last_error()
    same(f"allreduce commute={commute}", got, spec_value(L, 0, p, rank, commute, N, 4, xs))
    for root in (0, p - 1):
        got = np.full(N, SENT)
        assert L.MPI_Reduce(xs[rank].ctypes.data, got.ctypes.data, N, U, op.value, root, W) == 0, msx.last_error()
        if rank == root:
            same(f"reduce root={root} commute={commute}", got, spec_value(L, 1, p, root, commute, N, 4, xs))
    xs = [x_of(r, p * N, 3 + commute) for r in range(p)]
    got = np.full(N, SENT)
    assert L.MPI_Reduce_scatter_block(xs[rank].ctypes.data, got.ctypes.data, N, U, op.value, W) == 0, msx.last_error()
    mine = slice(rank * N, (rank + 1) * N)
    if commute:     # each rank combines its own block of every contribution
        exp = spec_value(L, 2, p, rank, 1, p * N, 4, [x[mine] for x in xs])
    else:           # the allreduce of the whole vector, then block `rank`
        exp = spec_value(L, 2, p, rank, 0, p * N, 4, xs)[mine]
    same(f"reduce_scatter_block commute={commute}", got, exp)
    assert L.MPI_Op_free(ctypes.byref(op)) == 0
print("RESULT", rank, p, len(fails), fails, flush=True)
assert L.MPI_Finalize() == 0
'''


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


# p = 3, 5, 6, 7: folds and absent leaves; p = 4, 8: the full trees
@pytest.mark.parametrize("p", [2, 3, 4, 5, 6, 7, 8])
def test_spec_is_the_order_of_the_pairwise_path(p):
    port = _free_port()
    procs = []
    for r in range(p):
        env = dict(os.environ)
        env.update({"MSX_SIZE": str(p), "MSX_RANK": str(r), "MSX_BOOTSTRAP_PORT": str(port),
                    "MSX_BOOTSTRAP_ADDR": "127.0.0.1"})
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
    seen = set()
    for rc, o, e in outs:
        assert rc == 0, (o + e)[-3000:]
        line = [l for l in o.splitlines() if l.startswith("RESULT")][0].split(" ", 4)
        assert int(line[2]) == p and int(line[3]) == 0, o
        seen.add(int(line[1]))
    assert seen == set(range(p))
