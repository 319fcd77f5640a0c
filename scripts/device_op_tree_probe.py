"""The fused tree of the device-op kernel kit against its yardsticks, on one MI355X.

fp32 `in + inout` (the bare AddF32 of tests/devop_tree), p = 8 sources, at
32 MiB and at 64 MiB per source (the DRAM form), finite inputs.  Three kernels
on the SAME buffers, interleaved inside each of 5 rounds, HIP events on one
stream; per round a warm figure (2 untimed calls, then 10 back to back) and a
cold one (Infinity Cache flushed by a 1 GiB read + write before each of 5
launches, median):
  builtin_tree  msx_reduce_tree_dev with MPI_SUM
  kit_tree      msx_kit::tree through msx_reduce_tree_user_dev (full 8-leaf tree)
  kit_pairwise  the sequence it replaces: seven msx_kit::combine launches in
                the tree's order over the same blocks (which it overwrites)
(a) kit_tree against builtin_tree, held against the builtin's own spread
    between rounds; recorded, not gated.
(b) kit_tree against kit_pairwise: gated -- faster at both sizes, warm and
    cold, by more than the larger of the two spreads.  The bytes moved predict
    84 / 36 = 2.3x.
(c) MPI_Allreduce at p = 4 ranks on the one GPU, 16 MiB per rank: the op with
    the tree function against the same functor without one, in the same run.
    Host clock around the blocking call after a barrier, rank 0's figures.
    Recorded, not gated.
The three forms' results are compared bit for bit first.  Prints one JSON line;
--out FILE also writes it there.
usage: python scripts/device_op_tree_probe.py [--out FILE] [--rounds N]    (GPU only)"""
import ctypes
import json
import os
import socket
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "microsoft-mpi_amd"))

import torch  # noqa: E402

import msx  # noqa: E402

WORKER = "--allreduce-worker" in sys.argv
rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 5
L = msx.init(errors_return=True)
C = msx.C
K = ctypes.CDLL(os.path.join(REPO, "tests", "devop_tree", "build", "libdevop_tree_ops.so"))
K.devop_tree_add_f32_pairwise8.restype = ctypes.c_int
K.devop_tree_add_f32_pairwise8.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
dev = torch.device("cuda:0")
PEAK = 8000.0      # GB/s, the HBM figure the project's fractions use
NSRC = 8


def addr(name):
    return ctypes.cast(getattr(K, name), ctypes.c_void_p)


def tree_op(name, with_tree, commute):
    op = ctypes.c_int(0)
    rc = L.msx_op_create_device_tree(addr(name), addr(name + "_tree") if with_tree else None, commute, None,
                                     ctypes.byref(op))
    assert rc == 0, msx.last_error()
    return op.value


def summary(ts, nbytes=None):
    s = sorted(ts)
    med = s[len(s) // 2]
    out = {"us": [round(x * 1e3, 1) for x in ts], "med_us": round(med * 1e3, 1),
           "spread": round((s[-1] - s[0]) / med, 4)}
    if nbytes:
        out["frac_of_8TBs"] = round(nbytes / med / 1e6 / PEAK, 4)
    return out


def allreduce_worker():
    """(c): one of p ranks; rank 0 prints the figures."""
    r_, s_ = ctypes.c_int(), ctypes.c_int()
    L.MPI_Comm_rank(C.MPI_COMM_WORLD, ctypes.byref(r_))
    L.MPI_Comm_size(C.MPI_COMM_WORLD, ctypes.byref(s_))
    rank, p = r_.value, s_.value
    n = (16 << 20) // 4
    g = torch.Generator(device=dev).manual_seed(100 + rank)
    x = torch.randint(-2**31, 2**31 - 1, (n,), dtype=torch.int32, device=dev, generator=g)
    got = {k: torch.zeros(n, dtype=torch.int32, device=dev) for k in ("device_op", "tree_op")}
    torch.cuda.synchronize()
    ops = {"device_op": tree_op("devop_tree_nc_u32", False, 0), "tree_op": tree_op("devop_tree_nc_u32", True, 0)}
    ts = {k: [] for k in ops}
    for it in range(rounds + 1):                     # the first round warms up
        for k, op in ops.items():
            L.MPI_Barrier(C.MPI_COMM_WORLD)
            t0 = time.perf_counter()
            rc = L.MPI_Allreduce(x.data_ptr(), got[k].data_ptr(), n, C.MPI_UNSIGNED, op, C.MPI_COMM_WORLD)
            t1 = time.perf_counter()
            assert rc == 0, msx.last_error()
            if it:
                ts[k].append((t1 - t0) * 1e3)
    same = bool(torch.equal(got["device_op"], got["tree_op"]))
    if rank == 0:
        print("ALLREDUCE " + json.dumps({"p": p, "mib_per_rank": 16, "results_equal": same,
                                         **{k: summary(v) for k, v in ts.items()}}), flush=True)
    L.MPI_Finalize()
    sys.exit(0 if same else 1)


if WORKER:
    allreduce_worker()

from msx import probe  # noqa: E402

P = probe.lib()
stream = torch.cuda.Stream(dev)
torch.cuda.set_stream(stream)
sp = ctypes.c_void_p(stream.cuda_stream)
flush = torch.empty(1 << 30, dtype=torch.uint8, device=dev)


def flush_cache():
    P.msxp_hbm(probe.READ1, flush.data_ptr(), flush.data_ptr(), flush.numel(), sp)
    P.msxp_hbm(probe.WRITE1, flush.data_ptr(), flush.data_ptr(), flush.numel(), sp)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(reps):
        fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def measure_stream(runs, nbytes):
    warm = {k: [] for k in runs}
    cold = {k: [] for k in runs}
    for _ in range(rounds):
        for name, fn in runs.items():
            fn(); fn()
            warm[name].append(timed(fn, 10))
            ts = []
            for _ in range(5):
                flush_cache()
                ts.append(timed(fn, 1))
            cold[name].append(sorted(ts)[2])
    return {k: {"warm": summary(warm[k], nbytes[k]), "cold": summary(cold[k], nbytes[k])} for k in runs}


out = {"rounds": rounds, "p": NSRC, "mismatches": [], "b_gate_ok": True}
add_op = tree_op("devop_tree_add_f32", True, 1)
g = torch.Generator(device=dev).manual_seed(1)
for mib in (32, 64):
    n = (mib << 20) // 4
    x = [torch.rand(n, device=dev, generator=g) * 2 - 1 for _ in range(NSRC)]
    res = {k: torch.zeros(n, device=dev) for k in ("builtin_tree", "kit_tree")}
    flat = (ctypes.c_void_p * NSRC)(*[t.data_ptr() for t in x])            # builtin: p sources
    slots = (ctypes.c_void_p * 32)()                                       # tree function: leaf k in slot 2k
    for k in range(NSRC):
        slots[2 * k] = x[k].data_ptr()

    def builtin_tree(n=n, flat=flat, o=res["builtin_tree"]):
        return L.msx_reduce_tree_dev(flat, NSRC, o.data_ptr(), n, C.MPI_FLOAT, C.MPI_SUM, sp)

    def kit_tree(n=n, slots=slots, o=res["kit_tree"]):
        return L.msx_reduce_tree_user_dev(slots, NSRC, 0, 0, 0, 0, o.data_ptr(), n, C.MPI_FLOAT, add_op, sp)

    def kit_pairwise(n=n, flat=flat):
        return K.devop_tree_add_f32_pairwise8(flat, n, sp)

    torch.cuda.synchronize()
    assert builtin_tree() == 0 and kit_tree() == 0, msx.last_error()
    assert kit_pairwise() == 0                                           # x[0] <- the tree's value
    torch.cuda.synchronize()
    if not torch.equal(res["builtin_tree"].view(torch.int32), res["kit_tree"].view(torch.int32)):
        out["mismatches"].append(["kit tree against builtin tree", mib])
    if not torch.equal(x[0].view(torch.int32), res["kit_tree"].view(torch.int32)):
        out["mismatches"].append(["kit tree against pairwise sequence", mib])
    size = mib << 20
    runs = {"builtin_tree": builtin_tree, "kit_tree": kit_tree, "kit_pairwise": kit_pairwise}
    nbytes = {"builtin_tree": (NSRC + 1) * size, "kit_tree": (NSRC + 1) * size, "kit_pairwise": 3 * (NSRC - 1) * size}
    m = measure_stream(runs, nbytes)
    for mode in ("warm", "cold"):
        b, t, q = (m[k][mode] for k in ("builtin_tree", "kit_tree", "kit_pairwise"))
        m[f"a_{mode}_kit_over_builtin"] = round(t["med_us"] / b["med_us"], 4)
        m[f"a_{mode}_within_builtin_spread"] = abs(t["med_us"] / b["med_us"] - 1) <= b["spread"]
        m[f"b_{mode}_pairwise_over_tree"] = round(q["med_us"] / t["med_us"], 3)
        ok = q["med_us"] / t["med_us"] - 1 > max(t["spread"], q["spread"])
        m[f"b_{mode}_faster_beyond_spread"] = ok
        out["b_gate_ok"] = out["b_gate_ok"] and ok
    out[f"tree_p8_{mib}mib"] = m
    del x, res, runs
    torch.cuda.empty_cache()
del flush
torch.cuda.empty_cache()

# ---- (c) allreduce at p = 4 on this GPU ---------------------------------------------
s = socket.socket()
s.bind(("127.0.0.1", 0))
port = s.getsockname()[1]
s.close()
procs = []
for r in range(4):
    env = dict(os.environ)
    env.update({"MSX_SIZE": "4", "MSX_RANK": str(r), "MSX_DEVICE": "0", "MSX_BOOTSTRAP_PORT": str(port),
                "MSX_BOOTSTRAP_ADDR": "127.0.0.1", "MSX_BOOTSTRAP_TIMEOUT": "180"})
    procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), "--allreduce-worker", "--rounds",
                                   str(rounds)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env))
for r, pr in enumerate(procs):
    try:
        o, e = pr.communicate(timeout=240)
    except subprocess.TimeoutExpired:
        pr.kill()
        o, e = pr.communicate()
    if pr.returncode != 0:
        out["mismatches"].append(["allreduce rank", r, pr.returncode, (o + e)[-400:]])
    for line in o.splitlines():
        if line.startswith("ALLREDUCE "):
            out["c_allreduce_p4_16mib"] = json.loads(line[len("ALLREDUCE "):])

text = json.dumps(out)
print(text)
if "--out" in sys.argv:
    path = sys.argv[sys.argv.index("--out") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
sys.exit(1 if out["mismatches"] or not out["b_gate_ok"] else 0)
