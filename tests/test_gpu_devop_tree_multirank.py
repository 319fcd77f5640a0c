"""GPU: the reduction collectives with a device user op that has a fused tree
function (msx_op_create_device_tree), p ranks on one GPU.

Every call is made on the same inputs with the tree op, with the same functor
registered without a tree (the pairwise path, which is the definition), with an
op whose tree function always declines, and with the host twin; the bytes must
be equal.  in (op) inout = 3 * in - inout (wrapping) is neither commutative nor
associative, so a swapped role or another association changes bits -- under
both commutative flags.  The ops library's counters show what ran: with the
tree op exactly one tree call of `count` elements on each evaluating rank and no
pairwise call (MPI_Scan / MPI_Exscan: pairwise calls within the bound of
DESIGN.md section 4 and no tree call); the op without a tree and the declining
op make the same pairwise calls as each other."""
import os
import subprocess
import sys
import textwrap

import pytest

import msx
from test_gpu_multirank import _assert_all_ranks, _free_port

pytestmark = pytest.mark.gpu
REPO = msx.REPO_ROOT

WORKER = r'''
import ctypes, os, sys
sys.path.insert(0, os.path.join(REPO, "microsoft-mpi_amd")); sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np, torch
import msx
from _xfer import todev, fromdev
C = msx.C
L = msx.init(errors_return=True)
K = ctypes.CDLL(os.path.join(REPO, "tests", "devop_tree", "build", "libdevop_tree_ops.so"))
K.devop_tree_stats.restype = None
K.devop_tree_stats.argtypes = [ctypes.POINTER(ctypes.c_int64), ctypes.c_int]
r_, s_ = ctypes.c_int(), ctypes.c_int()
L.MPI_Comm_rank(C.MPI_COMM_WORLD, ctypes.byref(r_)); L.MPI_Comm_size(C.MPI_COMM_WORLD, ctypes.byref(s_))
rank, p = r_.value, s_.value
W, U = C.MPI_COMM_WORLD, C.MPI_UNSIGNED
fails = []
COUNTS = [int(c) for c in os.environ["DEVOP_COUNTS"].split(",")]

def addr(name):
    return ctypes.cast(getattr(K, name), ctypes.c_void_p)

def tree_op(tree, commute):
    op = ctypes.c_int(0)
    assert L.msx_op_create_device_tree(addr("devop_tree_nc_u32"), addr(tree) if tree else None, commute, None,
                                       ctypes.byref(op)) == 0, msx.last_error()
    return op

def host_op(name, commute):
    op = ctypes.c_int(0)
    assert L.MPI_Op_create(addr(name), commute, ctypes.byref(op)) == 0, msx.last_error()
    return op

def stats():
    out = (ctypes.c_int64 * 6)()
    K.devop_tree_stats(out, 1)
    return list(out)       # pairwise calls, pairwise elements, tree calls, tree elements, on device, declined

def x_of(r, n, seed):
    i = np.arange(n, dtype=np.int64)
    base = (((i * 7 + r * 13) % 17) - 8).astype(np.int64).astype(np.uint32)
    return base ^ np.random.default_rng([seed, r]).integers(0, 2**32, n, dtype=np.uint32)

SENT = np.uint32(0xA5A5A5A5)

def same(tag, got, exp):
    if got.tobytes() != exp.tobytes():
        bad = np.nonzero(got != exp)[0] if got.size == exp.size else []
        fails.append(f"{tag} [{len(bad)} differ" + (f", first {bad[0]}" if len(bad) else "") + "]")

def builtin_sum(tag):
    # the window protocol is left consistent for the next user
    a = todev(np.full(257, rank + 1, np.int32))
    o = todev(np.zeros(257, np.int32))
    rc = L.MPI_Allreduce(a.data_ptr(), o.data_ptr(), 257, C.MPI_INT, C.MPI_SUM, W)
    got = fromdev(o, np.zeros(257, np.int32))
    if rc != 0 or not (got == p * (p + 1) // 2).all():
        fails.append(f"builtin MPI_SUM after {tag}: rc={rc}")

# each collective: make(n, seed) -> (run(op) -> (rc, result as uint32), the count
# its one evaluation covers on this rank (0: this rank evaluates nothing), fused?)
def run_allreduce(n, seed):
    x = x_of(rank, n, seed)
    def run(op):
        sb, rb = todev(x), todev(np.full(n, SENT))
        rc = L.MPI_Allreduce(sb.data_ptr(), rb.data_ptr(), n, U, op, W)
        return rc, fromdev(rb, x)
    return run, n, True

def run_iallreduce(n, seed):
    x = x_of(rank, n, seed)
    def run(op):
        sb, rb = todev(x), todev(np.full(n, SENT))
        req = ctypes.c_int(0)
        rc = L.MPI_Iallreduce(sb.data_ptr(), rb.data_ptr(), n, U, op, W, ctypes.byref(req))
        st = (ctypes.c_int * 8)()
        if rc == 0:
            rc = L.MPI_Wait(ctypes.byref(req), st)
        return rc, fromdev(rb, x)
    return run, n, True

def run_reduce(root):
    def make(n, seed):
        x = x_of(rank, n, seed)
        def run(op):
            sb, rb = todev(x), todev(np.full(n, SENT))
            rc = L.MPI_Reduce(sb.data_ptr(), rb.data_ptr(), n, U, op, root, W)
            return rc, fromdev(rb, x)
        return run, (n if rank == root else 0), True
    return make

def run_rs_block(n, seed, commute):
    x = x_of(rank, p * n, seed)
    def run(op):
        sb, rb = todev(x), todev(np.full(n, SENT))
        rc = L.MPI_Reduce_scatter_block(sb.data_ptr(), rb.data_ptr(), n, U, op, W)
        return rc, fromdev(rb, x, n)
    return run, (n if commute else p * n), True

def run_rs_ragged(n, seed, commute):
    counts = [(n + r) if r != 1 else n // 2 for r in range(p)]    # ragged; rank 1 gets nothing at n = 1
    total, mine = sum(counts), counts[rank]
    x = x_of(rank, total, seed)
    cc = (ctypes.c_int * p)(*counts)
    def run(op):
        sb, rb = todev(x), todev(np.full(max(mine, 1), SENT))
        rc = L.MPI_Reduce_scatter(sb.data_ptr(), rb.data_ptr(), cc, U, op, W)
        return rc, fromdev(rb, x, max(mine, 1))
    return run, (mine if commute else total), True

def run_scan(exclusive):
    def make(n, seed):
        x = x_of(rank, n, seed)
        def run(op):
            sb, rb = todev(x), todev(np.full(n, SENT))
            rc = (L.MPI_Exscan if exclusive else L.MPI_Scan)(sb.data_ptr(), rb.data_ptr(), n, U, op, W)
            return rc, fromdev(rb, x)
        return run, n, False
    return make

seed = 100
for commute in (0, 1):
    top, pop = tree_op("devop_tree_nc_u32_tree", commute), tree_op(None, commute)
    dop, hop = tree_op("devop_tree_decline", commute), host_op("devop_tree_nc_u32_host", commute)
    assert L.msx_op_has_device_tree(top.value) == 1 and L.msx_op_has_device_tree(pop.value) == 0
    cases = []
    for n in COUNTS:
        cases += [(n, "allreduce", run_allreduce), (n, "reduce root 0", run_reduce(0)),
                  (n, "reduce root p-1", run_reduce(p - 1)),
                  (n, "reduce_scatter_block", lambda n, s: run_rs_block(n, s, commute)),
                  (n, "reduce_scatter ragged", lambda n, s: run_rs_ragged(n, s, commute)),
                  (n, "scan", run_scan(False)), (n, "exscan", run_scan(True)), (n, "iallreduce", run_iallreduce)]
    if p == 4 and commute:
        # 4 x 32,768 uint32 = 512 KiB in all: the commutative gate takes the pairwise chain
        cases.append((32768, "reduce_scatter_block chain", lambda n, s: run_rs_block(n, s, 1)))
    for n, name, make in cases:
        seed += 1
        tag = f"{name} n={n} commute={commute}"
        run, count, fused = make(n, seed)
        stats()
        rc, got = run(top.value)
        pc, pe, tc, te, on_dev, declined = stats()
        if rc != 0:
            fails.append(f"{tag}: tree op rc={rc} {msx.last_error()}")
            continue
        if on_dev != 1:
            fails.append(f"{tag}: a function saw host memory")
        if fused and (pc, pe, tc, te) != ((0, 0, 1, count) if count else (0, 0, 0, 0)):
            fails.append(f"{tag}: tree op made {tc} tree calls of {te} elements and {pc} pairwise calls of {pe}, "
                         f"one tree call of {count} is due")
        if not fused and (tc != 0 or pe > 2 * (p - 1) * n):
            fails.append(f"{tag}: tree op made {tc} tree calls and {pe} pairwise elements")
        builtin_sum(tag)
        rc, plain = run(pop.value)
        plain_stats = stats()
        if rc != 0 or plain_stats[2:4] != [0, 0] or plain_stats[5] != 0:
            fails.append(f"{tag}: op without a tree: rc={rc} stats={plain_stats} {msx.last_error()}")
            continue
        if count and plain_stats[1] > (2 if not fused else 1) * (p - 1) * count:
            fails.append(f"{tag}: op without a tree: work {plain_stats} exceeds the bound")
        same(tag + " tree op against pairwise op", got, plain)
        rc, dec = run(dop.value)
        dec_stats = stats()
        if rc != 0 or dec_stats[:4] != plain_stats[:4] or dec_stats[5] != (1 if fused and count else 0):
            fails.append(f"{tag}: declining op: rc={rc} stats={dec_stats}, pairwise op {plain_stats} {msx.last_error()}")
            continue
        same(tag + " declining op against pairwise op", dec, plain)
        builtin_sum(tag + " declined")
        rc, exp = run(hop.value)
        if rc != 0:
            fails.append(f"{tag}: host op rc={rc} {msx.last_error()}")
            continue
        same(tag + " tree op against host twin", got, exp)
    for o in (top, pop, dop, hop):
        assert L.MPI_Op_free(ctypes.byref(o)) == 0

# a failing tree function fails the collective with its class
bad = tree_op("devop_tree_fail", 1)
x = x_of(rank, 100, 5)
sb, rb = todev(x), todev(np.full(100, SENT))
rc = L.MPI_Allreduce(sb.data_ptr(), rb.data_ptr(), 100, U, bad.value, W)
if rc != C.MPI_ERR_ARG:
    fails.append(f"failing tree function: rc={rc}")
stats()
builtin_sum("failing tree function")
assert L.MPI_Op_free(ctypes.byref(bad)) == 0

print("RESULT", rank, p, len(fails), fails[:16], flush=True)
L.MPI_Finalize()
'''


# p = 3 with 64-KiB windows: sub-slots of 20,480 bytes, so 13,000 uint32 take
# three gather chunks with a ragged last one
@pytest.mark.parametrize("p,chunk,counts", [(2, None, "1,1000"), (3, 65536, "1,1000,13000"), (4, None, "1,1000"),
                                            (6, None, "1000"), (8, None, "1000")])
def test_device_tree_op_collectives_p_ranks_on_one_gpu(p, chunk, counts):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    port = _free_port()
    procs = []
    for r in range(p):
        env = dict(os.environ)
        env.update({"MSX_SIZE": str(p), "MSX_RANK": str(r), "MSX_DEVICE": "0",
                    "MSX_BOOTSTRAP_PORT": str(port), "MSX_BOOTSTRAP_ADDR": "127.0.0.1",
                    "MSX_BOOTSTRAP_TIMEOUT": "180", "DEVOP_COUNTS": counts})
        if chunk:
            env["MSX_CHUNK_BYTES"] = str(chunk)
        procs.append(subprocess.Popen([sys.executable, "-c", f"REPO={REPO!r}\n" + textwrap.dedent(WORKER)],
                                      stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env))
    results = []
    for pr in procs:
        try:
            o, e = pr.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            pr.kill()
            o, e = pr.communicate()
        results.append((pr.returncode, o, e))
    _assert_all_ranks(results)
