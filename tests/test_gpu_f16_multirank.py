"""GPU: MSX_FLOAT16 / MSX_BFLOAT16 through the collectives and one RMA epoch,
p ranks on one GPU (launched like tests/test_gpu_multirank.py).

Two checks per call, neither against the library's own 16-bit output:
  order-free   rank-dependent small integers ((i*7 + rank*13) % 17 - 8, exactly
               representable, every partial sum below 256) against the closed
               form, and MAX on random bit patterns (NaNs and -0 taken out:
               with them MAX depends on the operand roles) against numpy's
               maximum -- duplicated or misrouted contributions fail here;
  order-exact  random finite inputs; expected = the numpy combine of
               tests/_half_ref.py walked over the association the schedule
               introspection (msx_schedule_algo_dt / _tree / _block, pinned to
               the oracle by tests/test_collectives_cpu.py) reports for that p,
               count and rank -- a tree that keeps an unrounded partial, or
               combines in another order, fails here.
MPI_Scan has no schedule introspection, so it gets the order-free checks only.
"""
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
import _half_ref as R
from _xfer import todev, fromdev
C = msx.C
L = msx.init(errors_return=True)
r_, s_ = ctypes.c_int(), ctypes.c_int()
L.MPI_Comm_rank(C.MPI_COMM_WORLD, ctypes.byref(r_)); L.MPI_Comm_size(C.MPI_COMM_WORLD, ctypes.byref(s_))
rank, p = r_.value, s_.value
fails = []
u16 = np.zeros(1, np.uint16)
IN_PLACE = ctypes.c_void_p(-1 & 0xffffffffffffffff)

def check(tag, got, exp):
    if got.tobytes() != exp.tobytes():
        bad = np.nonzero(got != exp)[0]
        fails.append(f"{tag} [{bad.size} differ, first {int(bad[0])}: got {int(got[bad[0]]):#06x} "
                     f"exp {int(exp[bad[0]]):#06x}]")

def dzeros(n):
    t = torch.zeros(max(2 * n, 2), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return t

def to_bits(dt, f):
    """Exactly representable fp32 values -> 16-bit patterns."""
    f = np.asarray(f, np.float32)
    if dt == "MSX_FLOAT16":
        b = f.astype(np.float16).view(np.uint16)
    else:
        b = (f.view(np.uint32) >> 16).astype(np.uint16)
    assert np.array_equal(R.W[dt](b), f)
    return b

def small(r, n):
    i = np.arange(n, dtype=np.int64)
    return ((i * 7 + r * 13) % 17 - 8).astype(np.float32)

def finite_bits(dt, seed, n):
    x = np.random.default_rng(seed).integers(0, 1 << 16, n, dtype=np.uint32).astype(np.uint16)
    inf = 0x7C00 if dt == "MSX_FLOAT16" else 0x7F80
    nf = (x & inf) == inf
    x[nf] ^= 0x0400 if dt == "MSX_FLOAT16" else 0x0080
    return x

def ordered_bits(dt, seed, n):
    x = finite_bits(dt, seed, n)
    x[x == 0x8000] = 0
    return x

def np_max(dt, xs):
    w = np.stack([R.W[dt](x) for x in xs])
    k = np.argmax(w, axis=0)
    out = np.stack(xs)[k, np.arange(xs[0].size)]
    assert np.array_equal(R.W[dt](out), w.max(axis=0))
    return out

# ---- schedule introspection -> association (as tests/test_collectives_cpu.py) ----
L.msx_schedule_tree.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p] * 4
L.msx_schedule_block.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
L.msx_schedule_algo_dt.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int]

def schedule_tree(which, pp, n):
    src = (ctypes.c_int * 32)()
    P, pm, ch = ctypes.c_int(), ctypes.c_uint(), ctypes.c_int()
    assert L.msx_schedule_tree(which, pp, n, src, ctypes.byref(P), ctypes.byref(pm), ctypes.byref(ch)) == 0
    return list(src), P.value, pm.value, bool(ch.value)

def schedule_block(pp, count, n):
    s, ln = ctypes.c_int64(), ctypes.c_int64()
    L.msx_schedule_block(pp, count, n, ctypes.byref(s), ctypes.byref(ln))
    return s.value, ln.value

def newrank(r, pp):
    return L.msx_schedule_newrank(r, pp)

def eval_tree(tree, xs, op, dt, lo, hi):
    src, P, pm, chain = tree
    if chain:
        v = xs[src[0]][lo:hi].copy()
        for k in range(1, P):
            v = R.combine(op, dt, v, xs[src[k]][lo:hi])
        return v
    leaves = []
    for k in range(P):
        if src[2 * k] < 0:
            leaves.append(None)
            continue
        v = xs[src[2 * k]][lo:hi].copy()
        if (pm >> k) & 1:
            v = R.combine(op, dt, v, xs[src[2 * k + 1]][lo:hi])
        leaves.append(v)
    w = 1
    while w < P:
        for k in range(0, P, 2 * w):
            if leaves[k + w] is not None:
                leaves[k] = R.combine(op, dt, leaves[k], leaves[k + w])
        w *= 2
    return leaves[0]

def exp_allreduce(xs, op, dt, r, nbc):
    count = xs[0].size
    n = newrank(r, p)
    if L.msx_schedule_algo_dt(0, p, count, getattr(C, dt), nbc) == 0:
        nn = n if n >= 0 else newrank(r + 1, p)
        return eval_tree(schedule_tree(0, p, nn), xs, op, dt, 0, count)
    out = np.empty_like(xs[0])
    pof2 = 1 << (p.bit_length() - 1)
    for m in range(pof2):
        lo, ln = schedule_block(p, count, m)
        out[lo:lo + ln] = eval_tree(schedule_tree(0, p, m), xs, op, dt, lo, lo + ln)
    return out

def exp_reduce(xs, op, dt, root):
    count = xs[0].size
    if L.msx_schedule_algo_dt(2, p, count, getattr(C, dt), 0) == 4:
        return eval_tree(schedule_tree(4, p, root), xs, op, dt, 0, count)
    out = np.empty_like(xs[0])
    pof2 = 1 << (p.bit_length() - 1)
    for m in range(pof2):
        lo, ln = schedule_block(p, count, m)
        out[lo:lo + ln] = eval_tree(schedule_tree(3, p, m), xs, op, dt, lo, lo + ln)
    return out

def exp_reduce_scatter_block(xs, per, op, dt, r):
    if L.msx_schedule_algo_dt(1, p, per * p, getattr(C, dt), 0) == 3:
        t = schedule_tree(2, p, r)
    else:
        n = newrank(r, p)
        t = schedule_tree(1, p, n if n >= 0 else newrank(r + 1, p))
    return eval_tree(t, xs, op, dt, r * per, (r + 1) * per)

L.MPI_Scan.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]
root = p - 1
algos = set()
# 1001 and 70001 elements sit on both sides of the MPI_Reduce (64 KiB) and
# reduce_scatter (512 KiB in all) switches; 2-byte elements cross the allreduce
# switch (256 KiB) only above 131072, so 140001 is added for the allreduces
for ci, count in enumerate((1001, 70001, 140001)):
    for dt in R.TYPES:
        D = getattr(C, dt)
        seed = 100 * count + (7 if dt == "MSX_FLOAT16" else 11)
        # the three input families, every rank's copy of every rank's vector
        ints = [to_bits(dt, small(r, count)) for r in range(p)]
        int_sum = to_bits(dt, sum(small(r, count) for r in range(p)))
        mx = [ordered_bits(dt, seed + r, count) for r in range(p)]
        mx_exp = np_max(dt, mx)
        fin = [finite_bits(dt, seed + 50 + r, count) for r in range(p)]
        algos.add((count, L.msx_schedule_algo_dt(0, p, count, D, 0)))
        for tag, xs, op, exp_fn in (
                ("ints", ints, "MPI_SUM", lambda r, nbc: int_sum),
                ("maxbits", mx, "MPI_MAX", lambda r, nbc: mx_exp),
                ("exact", fin, "MPI_SUM", lambda r, nbc: exp_allreduce(fin, "MPI_SUM", dt, r, nbc))):
            O = getattr(C, op)
            sb, rb = todev(xs[rank]), dzeros(count)
            rc = L.MPI_Allreduce(sb.data_ptr(), rb.data_ptr(), count, D, O, C.MPI_COMM_WORLD)
            if rc: fails.append(f"allreduce {tag} {dt} {count} rc={rc} {msx.last_error()}")
            else: check(f"allreduce {tag} {dt} {count}", fromdev(rb, u16, count), exp_fn(rank, 0))
            rb = dzeros(count)
            req = ctypes.c_int()
            rc = L.MPI_Iallreduce(sb.data_ptr(), rb.data_ptr(), count, D, O, C.MPI_COMM_WORLD, ctypes.byref(req))
            rc = rc or L.MPI_Wait(ctypes.byref(req), ctypes.c_void_p(1))
            if rc: fails.append(f"iallreduce {tag} {dt} {count} rc={rc} {msx.last_error()}")
            else: check(f"iallreduce {tag} {dt} {count}", fromdev(rb, u16, count), exp_fn(rank, 1))
        if count > 70001:
            continue
        # MPI_Reduce at a non-zero root
        for tag, xs, op, exp in (("ints", ints, "MPI_SUM", int_sum), ("maxbits", mx, "MPI_MAX", mx_exp),
                                 ("exact", fin, "MPI_SUM", None)):
            sb, rb = todev(xs[rank]), dzeros(count)
            rc = L.MPI_Reduce(sb.data_ptr(), rb.data_ptr(), count, D, getattr(C, op), root, C.MPI_COMM_WORLD)
            if rc: fails.append(f"reduce {tag} {dt} {count} rc={rc} {msx.last_error()}")
            elif rank == root:
                check(f"reduce {tag} {dt} {count}", fromdev(rb, u16, count),
                      exp if exp is not None else exp_reduce(fin, "MPI_SUM", dt, root))
        # MPI_Reduce_scatter_block: `count` elements per rank
        per = count
        ints_b = [to_bits(dt, small(r, per * p)) for r in range(p)]
        sum_b = to_bits(dt, sum(small(r, per * p) for r in range(p)))
        fin_b = [finite_bits(dt, seed + 80 + r, per * p) for r in range(p)]
        for tag, xs, exp in (("ints", ints_b, sum_b[rank * per:(rank + 1) * per]), ("exact", fin_b, None)):
            sb, rb = todev(xs[rank]), dzeros(per)
            rc = L.MPI_Reduce_scatter_block(sb.data_ptr(), rb.data_ptr(), per, D, C.MPI_SUM, C.MPI_COMM_WORLD)
            if rc: fails.append(f"rsb {tag} {dt} {per} rc={rc} {msx.last_error()}")
            else:
                check(f"rsb {tag} {dt} {per}", fromdev(rb, u16, per),
                      exp if exp is not None else exp_reduce_scatter_block(fin_b, per, "MPI_SUM", dt, rank))
        # MPI_Scan: order-free checks
        pre = to_bits(dt, sum(small(r, count) for r in range(rank + 1)))
        for tag, xs, op, exp in (("ints", ints, "MPI_SUM", pre), ("maxbits", mx, "MPI_MAX", np_max(dt, mx[:rank + 1]))):
            sb, rb = todev(xs[rank]), dzeros(count)
            rc = L.MPI_Scan(sb.data_ptr(), rb.data_ptr(), count, D, getattr(C, op), C.MPI_COMM_WORLD)
            if rc: fails.append(f"scan {tag} {dt} {count} rc={rc} {msx.last_error()}")
            else: check(f"scan {tag} {dt} {count}", fromdev(rb, u16, count), exp)

# one MPI_Accumulate fence epoch: every rank adds small integers into rank 0's
# window and random finite bits (MAX-free SUM, order self first then ascending
# as tests/test_gpu_rma.py pins it) into the last rank's
K = 1001
for dt in R.TYPES:
    D = getattr(C, dt)
    init0 = to_bits(dt, small(31, 2 * K))
    initl = finite_bits(dt, 900, 2 * K)
    wt = todev(init0 if rank == 0 else initl if rank == p - 1 else np.zeros(2 * K, np.uint16))
    if p == 1:
        wt = todev(init0)
    win = ctypes.c_int()
    assert L.MPI_Win_create(wt.data_ptr(), 4 * K, 2, C.MPI_INFO_NULL, C.MPI_COMM_WORLD, ctypes.byref(win)) == 0
    L.MPI_Win_set_errhandler(win, C.MPI_ERRORS_RETURN)
    rc = L.MPI_Win_fence(0, win)
    a_int = todev(to_bits(dt, small(rank, K)))
    a_fin = todev(finite_bits(dt, 950 + rank, K))
    rc = rc or L.MPI_Accumulate(a_int.data_ptr(), K, D, 0, 3, K, D, C.MPI_SUM, win)
    if p > 1:
        rc = rc or L.MPI_Accumulate(a_fin.data_ptr(), K, D, p - 1, 5, K, D, C.MPI_SUM, win)
    rc = rc or L.MPI_Win_fence(0, win)
    if rc:
        fails.append(f"accumulate epoch {dt} rc={rc} {msx.last_error()}")
    else:
        got = fromdev(wt, u16, 2 * K)
        if rank == 0:
            exp = init0.copy()
            exp[3:3 + K] = to_bits(dt, R.W[dt](init0[3:3 + K]) + sum(small(r, K) for r in range(p)))
            check(f"accumulate ints {dt}", got, exp)
        if rank == p - 1 and p > 1:
            exp = initl.copy()
            for o in [p - 1] + list(range(p - 1)):
                exp[5:5 + K] = R.combine("MPI_SUM", dt, exp[5:5 + K].copy(), finite_bits(dt, 950 + o, K))
            check(f"accumulate exact {dt}", got, exp)
    L.MPI_Win_free(ctypes.byref(win))

print("ALGOS", sorted(algos), flush=True)
print("RESULT", rank, p, len(fails), fails[:8], flush=True)
L.MPI_Finalize()
'''


@pytest.mark.parametrize("p", [3, 8])
def test_half_collectives_p_ranks_on_one_gpu(p):
    """p = 3: the non-power-of-two fold; p = 8: the full tree.  Counts 1001 and
    70001 (plus 140001 for the allreduces): both sides of every
    recursive-doubling / Rabenseifner / pairwise switch, block boundaries at
    addresses that are not 16-byte aligned."""
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    port = _free_port()
    procs = []
    for r in range(p):
        env = dict(os.environ)
        env.update({"MSX_SIZE": str(p), "MSX_RANK": str(r), "MSX_DEVICE": "0",
                    "MSX_BOOTSTRAP_PORT": str(port), "MSX_BOOTSTRAP_ADDR": "127.0.0.1",
                    "MSX_BOOTSTRAP_TIMEOUT": "180"})
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
    # recursive doubling (0) at the small count, Rabenseifner (1) at the largest
    algos = [l for l in results[0][1].splitlines() if l.startswith("ALGOS")]
    assert algos and "(1001, 0)" in algos[0] and "(140001, 1)" in algos[0], algos
