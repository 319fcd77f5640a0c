"""GPU: the reduction collectives with a device-resident user op, p ranks on
one GPU.

The host user-op path is the definition (tests/test_collectives_cpu.py pins it
to the reference's order): every call is made twice on the same buffers, once
with the device op devop_nc_u32 and once with its host twin, and the bytes must
be equal.  in (op) inout = 3 * in - inout (wrapping) is neither commutative nor
associative, so a swapped role or another association changes bits -- under
both commutative flags.  Per call the ops library's counters must stay within
the work bounds of DESIGN.md section 4 (one rank evaluates only its own
result), and every operand the function saw was device memory."""
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
K = ctypes.CDLL(os.path.join(REPO, "tests", "devop", "build", "libdevop_ops.so"))
K.devop_stats.restype = None
K.devop_stats.argtypes = [ctypes.POINTER(ctypes.c_int64), ctypes.c_int]
K.devop_set_stride2_n.restype = None
K.devop_set_stride2_n.argtypes = [ctypes.c_int]
r_, s_ = ctypes.c_int(), ctypes.c_int()
L.MPI_Comm_rank(C.MPI_COMM_WORLD, ctypes.byref(r_)); L.MPI_Comm_size(C.MPI_COMM_WORLD, ctypes.byref(s_))
rank, p = r_.value, s_.value
W, U = C.MPI_COMM_WORLD, C.MPI_UNSIGNED
fails = []
COUNTS = [int(c) for c in os.environ["DEVOP_COUNTS"].split(",")]

def addr(name):
    return ctypes.cast(getattr(K, name), ctypes.c_void_p)

def dev_op(name, commute):
    op = ctypes.c_int(0)
    assert L.msx_op_create_device(addr(name), commute, None, ctypes.byref(op)) == 0, msx.last_error()
    return op

def host_op(name, commute):
    op = ctypes.c_int(0)
    assert L.MPI_Op_create(addr(name), commute, ctypes.byref(op)) == 0, msx.last_error()
    return op

def stats():
    out = (ctypes.c_int64 * 3)()
    K.devop_stats(out, 1)
    return list(out)

def x_of(r, n, seed):
    i = np.arange(n, dtype=np.int64)
    base = (((i * 7 + r * 13) % 17) - 8).astype(np.int64).astype(np.uint32)
    return base ^ np.random.default_rng([seed, r]).integers(0, 2**32, n, dtype=np.uint32)

def nc(a, b):
    return (a * np.uint32(3) - b).astype(np.uint32)

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

# each collective: run(op) -> (rc, result bytes as uint32), fresh device buffers
def run_allreduce(n, seed):
    x = x_of(rank, n, seed)
    def run(op):
        sb, rb = todev(x), todev(np.full(n, SENT))
        rc = L.MPI_Allreduce(sb.data_ptr(), rb.data_ptr(), n, U, op, W)
        return rc, fromdev(rb, x)
    return run, (p - 1) * n

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
    return run, (p - 1) * n

def run_reduce(root):
    def make(n, seed):
        x = x_of(rank, n, seed)
        def run(op):
            sb, rb = todev(x), todev(np.full(n, SENT))
            rc = L.MPI_Reduce(sb.data_ptr(), rb.data_ptr(), n, U, op, root, W)
            return rc, fromdev(rb, x)
        return run, ((p - 1) * n if rank == root else 0)
    return make

def run_rs_block(n, seed, commute):
    x = x_of(rank, p * n, seed)
    def run(op):
        sb, rb = todev(x), todev(np.full(n, SENT))
        rc = L.MPI_Reduce_scatter_block(sb.data_ptr(), rb.data_ptr(), n, U, op, W)
        return rc, fromdev(rb, x, n)
    return run, ((p - 1) * n if commute else (p - 1) * p * n)

def run_rs_ragged(n, seed, commute):
    counts = [(n + r) if r != 1 else n // 2 for r in range(p)]    # ragged; rank 1 gets nothing at n = 1
    total, mine = sum(counts), counts[rank]
    x = x_of(rank, total, seed)
    cc = (ctypes.c_int * p)(*counts)
    def run(op):
        sb, rb = todev(x), todev(np.full(max(mine, 1), SENT))
        rc = L.MPI_Reduce_scatter(sb.data_ptr(), rb.data_ptr(), cc, U, op, W)
        return rc, fromdev(rb, x, max(mine, 1))
    return run, ((p - 1) * mine if commute else (p - 1) * total)

def run_scan(exclusive):
    def make(n, seed):
        x = x_of(rank, n, seed)
        def run(op):
            sb, rb = todev(x), todev(np.full(n, SENT))
            rc = (L.MPI_Exscan if exclusive else L.MPI_Scan)(sb.data_ptr(), rb.data_ptr(), n, U, op, W)
            return rc, fromdev(rb, x)
        return run, 2 * (p - 1) * n
    return make

seed = 100
for commute in (0, 1):
    dop, hop = dev_op("devop_nc_u32", commute), host_op("devop_nc_u32_host", commute)
    for n in COUNTS:
        cases = [("allreduce", run_allreduce), ("reduce root 0", run_reduce(0)), ("reduce root p-1", run_reduce(p - 1)),
                 ("reduce_scatter_block", lambda n, s: run_rs_block(n, s, commute)),
                 ("reduce_scatter ragged", lambda n, s: run_rs_ragged(n, s, commute)),
                 ("scan", run_scan(False)), ("exscan", run_scan(True)), ("iallreduce", run_iallreduce)]
        for name, make in cases:
            seed += 1
            tag = f"{name} n={n} commute={commute}"
            run, bound = make(n, seed)
            stats()
            rc, got = run(dop.value)
            calls, total, on_dev = stats()
            if rc != 0:
                fails.append(f"{tag}: device op rc={rc} {msx.last_error()}")
                continue
            if total > bound or (bound == 0 and calls != 0):
                fails.append(f"{tag}: work {total} elements in {calls} calls exceeds the bound {bound}")
            if on_dev != 1:
                fails.append(f"{tag}: the function saw host memory")
            builtin_sum(tag)
            rc, exp = run(hop.value)
            if rc != 0:
                fails.append(f"{tag}: host op rc={rc} {msx.last_error()}")
                continue
            same(tag, got, exp)
            if calls == 0 and (name in ("allreduce", "iallreduce") or (name.startswith("reduce root") and bound)):
                fails.append(f"{tag}: the device function was never called")
            # closed forms at p = 2 (host_user_allreduce / host_user_scan by hand)
            if p == 2 and name in ("allreduce", "iallreduce"):
                x0, x1 = x_of(0, n, seed), x_of(1, n, seed)
                want = nc(x0, x1) if not commute else nc(x_of(1 - rank, n, seed), x_of(rank, n, seed))
                same(tag + " closed form", got, want)
            if p == 2 and name == "scan":
                x0, x1 = x_of(0, n, seed), x_of(1, n, seed)
                same(tag + " closed form", got, x0 if rank == 0 else nc(x0, x1))
    assert L.MPI_Op_free(ctypes.byref(dop)) == 0 and L.MPI_Op_free(ctypes.byref(hop)) == 0

# pageable host send and receive buffers: staged to the device at the ends
dop, hop = dev_op("devop_nc_u32", 0), host_op("devop_nc_u32_host", 0)
n = 3001
x = x_of(rank, n, 7)
got, exp = np.full(n, SENT), np.full(n, SENT)
stats()
rc = L.MPI_Allreduce(x.ctypes.data, got.ctypes.data, n, U, dop.value, W)
calls, total, on_dev = stats()
if rc != 0 or on_dev != 1 or total > (p - 1) * n:
    fails.append(f"host buffers: rc={rc} on_device={on_dev} work={total} {msx.last_error()}")
rc = L.MPI_Allreduce(x.ctypes.data, exp.ctypes.data, n, U, hop.value, W)
same("allreduce host buffers", got, exp)
builtin_sum("host buffers")
assert L.MPI_Op_free(ctypes.byref(dop)) == 0 and L.MPI_Op_free(ctypes.byref(hop)) == 0

# a derived datatype with gaps: MPI_Type_vector(n, 1, 2, MPI_UNSIGNED), count 1
n = 777
t = ctypes.c_int()
assert L.MPI_Type_vector(n, 1, 2, U, ctypes.byref(t)) == 0 and L.MPI_Type_commit(ctypes.byref(t)) == 0
K.devop_set_stride2_n(n)
dop, hop = dev_op("devop_stride2_u32", 0), host_op("devop_stride2_u32_host", 0)
x = x_of(rank, 2 * n - 1, 8)
fill = x_of(rank + 100, 2 * n - 1, 9)            # what recvbuf holds before: its gaps must survive
sb, rb = todev(x), todev(fill)
stats()
rc = L.MPI_Allreduce(sb.data_ptr(), rb.data_ptr(), 1, t.value, dop.value, W)
calls, total, on_dev = stats()
if rc != 0 or on_dev != 1 or total > (p - 1):
    fails.append(f"stride2: rc={rc} on_device={on_dev} work={total} {msx.last_error()}")
got = fromdev(rb, x)
sb, rb = todev(x), todev(fill)
rc = L.MPI_Allreduce(sb.data_ptr(), rb.data_ptr(), 1, t.value, hop.value, W)
exp = fromdev(rb, x)
same("allreduce stride2", got, exp)
same("allreduce stride2 gaps", got[1::2], fill[1::2])
if (got[0::2] == fill[0::2]).all():
    fails.append("allreduce stride2: mapped elements were not written")
builtin_sum("stride2")
assert L.MPI_Op_free(ctypes.byref(dop)) == 0 and L.MPI_Op_free(ctypes.byref(hop)) == 0
assert L.MPI_Type_free(ctypes.byref(t)) == 0

# intercommunicator reductions refuse a device op, and say so
if p == 4:                                       # groups {0, 1} and {2, 3}
    low = rank < 2
    loc, ic = ctypes.c_int(), ctypes.c_int()
    assert L.MPI_Comm_split(W, 0 if low else 1, rank, ctypes.byref(loc)) == 0, msx.last_error()
    assert L.MPI_Intercomm_create(loc.value, 0, W, 2 if low else 0, 9, ctypes.byref(ic)) == 0, msx.last_error()
    assert L.MPI_Comm_set_errhandler(ic.value, C.MPI_ERRORS_RETURN) == 0
    dop = dev_op("devop_nc_u32", 1)
    sb, rb = todev(x_of(rank, 16, 10)), todev(np.full(16, SENT))
    stats()
    rc = L.MPI_Allreduce(sb.data_ptr(), rb.data_ptr(), 16, U, dop.value, ic.value)
    if rc != C.MPI_ERR_OP or "intercommunicator" not in msx.last_error() or stats()[0] != 0:
        fails.append(f"intercommunicator allreduce with a device op: rc={rc} {msx.last_error()}")
    assert L.MPI_Op_free(ctypes.byref(dop)) == 0
    assert L.MPI_Comm_free(ctypes.byref(ic)) == 0 and L.MPI_Comm_free(ctypes.byref(loc)) == 0

print("RESULT", rank, p, len(fails), fails[:16], flush=True)
L.MPI_Finalize()
'''


# p = 3 with 64-KiB windows: sub-slots of 20,480 bytes, so 13,000 uint32 take
# three gather chunks with a ragged last one
@pytest.mark.parametrize("p,chunk,counts", [(2, None, "1,1000"), (3, 65536, "1,1000,13000"), (4, None, "1,1000")])
def test_device_op_collectives_p_ranks_on_one_gpu(p, chunk, counts):
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
