"""GPU: MSX_SUM_WIDE through the collectives that accept it, p ranks on one GPU
(launched like tests/test_gpu_f16_multirank.py).

Two checks per call, neither against the library's own output:
  order-free   rank-dependent small integers ((i*7 + rank*13) % 17 - 8, exactly
               representable, every partial sum below 256) against the closed
               form -- duplicated or misrouted contributions fail here;
  order-exact  finite inputs (random patterns, every other element within a
               binade of 1 so that partial sums outgrow the mantissa); expected
               = the wide reference of tests/_wide_ref.py walked over the
               association the schedule introspection (msx_schedule_algo_dt /
               _tree / _block) reports for that p, count and rank.  Before each
               comparison the worker asserts in numpy that the per-node
               expectation of tests/_half_ref.py differs: a tree that rounds at
               every node fails.
MPI_Scan must refuse the op on every rank and leave the communicator usable.
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
import _wide_ref as WR
from _xfer import todev, fromdev
C = msx.C
WIDE = C.MSX_SUM_WIDE
L = msx.init(errors_return=True)
r_, s_ = ctypes.c_int(), ctypes.c_int()
L.MPI_Comm_rank(C.MPI_COMM_WORLD, ctypes.byref(r_)); L.MPI_Comm_size(C.MPI_COMM_WORLD, ctypes.byref(s_))
rank, p = r_.value, s_.value
fails = []
u16 = np.zeros(1, np.uint16)

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
    """Random finite patterns at the odd indices, magnitudes within a binade of
    1 (random sign and mantissa) at the even ones."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 1 << 16, n, dtype=np.uint32).astype(np.uint16)
    inf = 0x7C00 if dt == "MSX_FLOAT16" else 0x7F80
    nf = (x & inf) == inf
    x[nf] ^= 0x0400 if dt == "MSX_FLOAT16" else 0x0080
    mant, one = (10, 0x3C00) if dt == "MSX_FLOAT16" else (7, 0x3F80)
    k = (n + 1) // 2
    near = (one + (rng.integers(-1, 2, k) << mant) + rng.integers(0, 1 << mant, k)).astype(np.uint16)
    x[0::2] = near | (rng.integers(0, 2, k).astype(np.uint16) << 15)
    return x

# ---- schedule introspection -> association (as tests/test_gpu_f16_multirank.py) ----
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

def eval_tree(tree, xs, dt, lo, hi):
    """(wide expectation, per-node expectation) of one rank tree over [lo, hi)."""
    src, P, pm, chain = tree
    ns = P if chain else 2 * P
    srcs = [xs[r][lo:hi] if r >= 0 else None for r in src[:ns]]
    nl = 0
    if not chain:
        while nl < P and src[2 * nl] >= 0:
            nl += 1
        assert all(src[2 * k] < 0 for k in range(nl, P))       # absent leaves trail
    return WR.tree(dt, srcs, P, pm, nl, chain), R.tree("MPI_SUM", dt, srcs, P, pm, nl, chain)

def blocks(which, pp, xs, dt):
    count = xs[0].size
    out, pn = np.empty_like(xs[0]), np.empty_like(xs[0])
    pof2 = 1 << (pp.bit_length() - 1)
    for m in range(pof2):
        lo, ln = schedule_block(pp, count, m)
        out[lo:lo + ln], pn[lo:lo + ln] = eval_tree(schedule_tree(which, pp, m), xs, dt, lo, lo + ln)
    return out, pn

def exp_allreduce(xs, dt, r, nbc, pp):
    count = xs[0].size
    n = newrank(r, pp)
    if L.msx_schedule_algo_dt(0, pp, count, getattr(C, dt), nbc) == 0:
        nn = n if n >= 0 else newrank(r + 1, pp)
        return eval_tree(schedule_tree(0, pp, nn), xs, dt, 0, count)
    return blocks(0, pp, xs, dt)

def exp_reduce(xs, dt, root):
    count = xs[0].size
    if L.msx_schedule_algo_dt(2, p, count, getattr(C, dt), 0) == 4:
        return eval_tree(schedule_tree(4, p, root), xs, dt, 0, count)
    return blocks(3, p, xs, dt)

def exp_reduce_scatter_block(xs, per, dt, r):
    if L.msx_schedule_algo_dt(1, p, per * p, getattr(C, dt), 0) == 3:
        t = schedule_tree(2, p, r)
    else:
        n = newrank(r, p)
        t = schedule_tree(1, p, n if n >= 0 else newrank(r + 1, p))
    return eval_tree(t, xs, dt, r * per, (r + 1) * per)

def exact(tag, got, pair, nsrc):
    """Compare with the wide expectation, after the degenerate-input guard."""
    exp, per_node = pair
    if nsrc > 2 and not np.count_nonzero(exp != per_node) > 0:
        fails.append(f"{tag}: degenerate input, per-node rounding gives the same bytes")
    check(tag, got, exp)

L.MPI_Scan.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]
W = C.MPI_COMM_WORLD
root = p - 1
algos = set()
# 1001 and 70001 elements sit on both sides of the MPI_Reduce (64 KiB) and
# reduce_scatter (512 KiB in all) switches; 2-byte elements cross the allreduce
# switch (256 KiB) only above 131072, so 140001 is added for the allreduces
for count in (1001, 70001, 140001):
    for dt in R.TYPES:
        D = getattr(C, dt)
        seed = 100 * count + (7 if dt == "MSX_FLOAT16" else 11)
        ints = [to_bits(dt, small(r, count)) for r in range(p)]
        int_sum = to_bits(dt, sum(small(r, count) for r in range(p)))
        fin = [finite_bits(dt, seed + 50 + r, count) for r in range(p)]
        algos.add((count, L.msx_schedule_algo_dt(0, p, count, D, 0)))
        for tag, xs in (("ints", ints), ("exact", fin)):
            sb, rb = todev(xs[rank]), dzeros(count)
            rc = L.MPI_Allreduce(sb.data_ptr(), rb.data_ptr(), count, D, WIDE, W)
            if rc: fails.append(f"allreduce {tag} {dt} {count} rc={rc} {msx.last_error()}")
            elif tag == "ints": check(f"allreduce ints {dt} {count}", fromdev(rb, u16, count), int_sum)
            else: exact(f"allreduce exact {dt} {count}", fromdev(rb, u16, count), exp_allreduce(fin, dt, rank, 0, p), p)
            rb = dzeros(count)
            req = ctypes.c_int()
            rc = L.MPI_Iallreduce(sb.data_ptr(), rb.data_ptr(), count, D, WIDE, W, ctypes.byref(req))
            rc = rc or L.MPI_Wait(ctypes.byref(req), ctypes.c_void_p(1))
            if rc: fails.append(f"iallreduce {tag} {dt} {count} rc={rc} {msx.last_error()}")
            elif tag == "ints": check(f"iallreduce ints {dt} {count}", fromdev(rb, u16, count), int_sum)
            else: exact(f"iallreduce exact {dt} {count}", fromdev(rb, u16, count), exp_allreduce(fin, dt, rank, 1, p), p)
        if count > 70001:
            continue
        # MPI_Reduce at the last rank
        for tag, xs in (("ints", ints), ("exact", fin)):
            sb, rb = todev(xs[rank]), dzeros(count)
            rc = L.MPI_Reduce(sb.data_ptr(), rb.data_ptr(), count, D, WIDE, root, W)
            if rc: fails.append(f"reduce {tag} {dt} {count} rc={rc} {msx.last_error()}")
            elif rank == root and tag == "ints": check(f"reduce ints {dt} {count}", fromdev(rb, u16, count), int_sum)
            elif rank == root: exact(f"reduce exact {dt} {count}", fromdev(rb, u16, count), exp_reduce(fin, dt, root), p)
        # MPI_Reduce_scatter_block: `count` elements per rank
        per = count
        ints_b = [to_bits(dt, small(r, per * p)) for r in range(p)]
        sum_b = to_bits(dt, sum(small(r, per * p) for r in range(p)))
        fin_b = [finite_bits(dt, seed + 80 + r, per * p) for r in range(p)]
        for tag, xs in (("ints", ints_b), ("exact", fin_b)):
            sb, rb = todev(xs[rank]), dzeros(per)
            rc = L.MPI_Reduce_scatter_block(sb.data_ptr(), rb.data_ptr(), per, D, WIDE, W)
            if rc: fails.append(f"rsb {tag} {dt} {per} rc={rc} {msx.last_error()}")
            elif tag == "ints": check(f"rsb ints {dt} {per}", fromdev(rb, u16, per), sum_b[rank * per:(rank + 1) * per])
            else: exact(f"rsb exact {dt} {per}", fromdev(rb, u16, per), exp_reduce_scatter_block(fin_b, per, dt, rank), p)

K = 1001
for dt in R.TYPES:
    D = getattr(C, dt)
    fin = [finite_bits(dt, 4000 + r, K) for r in range(p)]
    # pageable host buffers
    sb, rb = fin[rank].copy(), np.zeros(K, np.uint16)
    rc = L.MPI_Allreduce(sb.ctypes.data, rb.ctypes.data, K, D, WIDE, W)
    if rc: fails.append(f"host allreduce {dt} rc={rc} {msx.last_error()}")
    else: exact(f"host allreduce {dt}", rb, exp_allreduce(fin, dt, rank, 0, p), p)
    # MPI_Scan / MPI_Exscan refuse the op on every rank, before any communication ...
    sd, rd = todev(fin[rank]), dzeros(K)
    for fn in (L.MPI_Scan, L.MPI_Exscan):
        rc = fn(sd.data_ptr(), rd.data_ptr(), K, D, WIDE, W)
        if rc != C.MPI_ERR_OP or "MSX_SUM_WIDE" not in msx.last_error():
            fails.append(f"scan {dt}: rc={rc} '{msx.last_error()}', expected MPI_ERR_OP naming the op")
    if fromdev(rd, u16, K).any(): fails.append(f"scan {dt}: the refused call wrote recvbuf")
    # ... and leave no protocol state behind: the next allreduce is exact
    rc = L.MPI_Allreduce(sd.data_ptr(), rd.data_ptr(), K, D, WIDE, W)
    if rc: fails.append(f"allreduce after scan {dt} rc={rc} {msx.last_error()}")
    else: exact(f"allreduce after scan {dt}", fromdev(rd, u16, K), exp_allreduce(fin, dt, rank, 0, p), p)
    # MPI_Comm_split halves (even / odd ranks) and a duplicate of one
    half, dup = ctypes.c_int(), ctypes.c_int()
    rc = L.MPI_Comm_split(W, rank % 2, rank, ctypes.byref(half))
    rc = rc or L.MPI_Comm_set_errhandler(half, C.MPI_ERRORS_RETURN)
    rc = rc or L.MPI_Comm_dup(half, ctypes.byref(dup))
    rc = rc or L.MPI_Comm_set_errhandler(dup, C.MPI_ERRORS_RETURN)
    if rc:
        fails.append(f"comm split/dup rc={rc} {msx.last_error()}")
        continue
    members = list(range(rank % 2, p, 2))
    sub = [fin[r] for r in members]
    for name, comm in (("split", half), ("dup", dup)):
        rd = dzeros(K)
        rc = L.MPI_Allreduce(sd.data_ptr(), rd.data_ptr(), K, D, WIDE, comm.value)
        if rc: fails.append(f"{name} allreduce {dt} rc={rc} {msx.last_error()}")
        elif len(members) == 1: check(f"{name} allreduce {dt}", fromdev(rd, u16, K), fin[rank])
        else:
            exact(f"{name} allreduce {dt}", fromdev(rd, u16, K),
                  exp_allreduce(sub, dt, members.index(rank), 0, len(members)), len(members))
    L.MPI_Comm_free(ctypes.byref(dup)); L.MPI_Comm_free(ctypes.byref(half))

st = (ctypes.c_double * 8)()
L.msx_engine_stats(st, 8, 0)
print("FLAGCALLS", int(st[7]), flush=True)
print("ALGOS", sorted(algos), flush=True)
print("RESULT", rank, p, len(fails), fails[:8], flush=True)
L.MPI_Finalize()
'''


@pytest.mark.parametrize("p,mode", [(3, None), (8, None), (4, "+ts")])
def test_wide_collectives_p_ranks_on_one_gpu(p, mode):
    """p = 3: the non-power-of-two fold; p = 8: the full tree, default
    schedules; p = 4 `+ts`: MSX_TWO_STEP_MAX set as the `+ts` cases of
    tests/test_gpu_multirank.py set it, so the flag small call, the two-step
    allreduce / reduce and the one-step reduce_scatter run.  Counts 1001 and
    70001 (plus 140001 for the allreduces): both sides of every algorithm
    switch, block boundaries at addresses that are not 16-byte aligned."""
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
        if mode == "+ts":
            env["MSX_TWO_STEP_MAX"] = str(1 << 62)
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
    flag_calls = [int(l.split()[1]) for l in results[0][1].splitlines() if l.startswith("FLAGCALLS")]
    if mode == "+ts":
        assert flag_calls and flag_calls[0] > 0, flag_calls      # the GPU-flag Rabenseifner schedules ran
