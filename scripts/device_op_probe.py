"""Device-resident user ops against their yardsticks, on one MI355X.

(a) the kernel kit (include/msx_device_op.h) with an fp32 `in + inout` functor
    through msx_reduce_local_dev, against the builtin MPI_SUM fp32 kernel, at
    256 MiB and at 4 MiB per operand.  HIP events on one stream, the two
    on the same operands, interleaved inside each of 5 rounds; per round a warm figure (2 untimed
    calls, then 10 back to back) and a cold one (Infinity Cache flushed by a
    1 GiB read + write before each of 5 launches, median).  The builtin's own
    spread between rounds is what a difference is held against.
(b) MPI_Reduce_local on 64 MiB device operands: the host-twin user op (staged
    to host memory and back) against the device op.  Blocking calls, host clock;
    per round a warm figure (2 untimed calls, then the median of 3) and a cold one.
(c) MPI_Allreduce at p = 4 ranks on the one GPU, 16 MiB per rank: host-twin op
    against device op.  Host clock around the blocking call after a barrier,
    rank 0's figures.
(b) and (c) are recorded, not gated.  The ops come from
tests/devop/build/libdevop_ops.so.  Prints one JSON line; --out FILE also
writes it there.
usage: python scripts/device_op_probe.py [--out FILE] [--rounds N]    (GPU only)"""
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
K = ctypes.CDLL(os.path.join(REPO, "tests", "devop", "build", "libdevop_ops.so"))
dev = torch.device("cuda:0")
PEAK = 8000.0      # GB/s, the HBM figure the project's fractions use


def addr(name):
    return ctypes.cast(getattr(K, name), ctypes.c_void_p)


def device_op(name, commute):
    op = ctypes.c_int(0)
    assert L.msx_op_create_device(addr(name), commute, None, ctypes.byref(op)) == 0, msx.last_error()
    return op.value


def host_op(name, commute):
    op = ctypes.c_int(0)
    assert L.MPI_Op_create(addr(name), commute, ctypes.byref(op)) == 0, msx.last_error()
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
    got = {k: torch.zeros(n, dtype=torch.int32, device=dev) for k in ("host_twin", "device_op")}
    torch.cuda.synchronize()
    ops = {"host_twin": host_op("devop_nc_u32_host", 0), "device_op": device_op("devop_nc_u32", 0)}
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
    same = bool(torch.equal(got["host_twin"], got["device_op"]))
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
    return {k: {"warm": summary(warm[k], nbytes), "cold": summary(cold[k], nbytes)} for k in runs}


out = {"rounds": rounds, "mismatches": []}

# ---- (a) kit fp32 add against builtin MPI_SUM fp32 ---------------------------------
add_op = device_op("devop_add_f32", 1)
g = torch.Generator(device=dev).manual_seed(1)
for mib in (256, 4):
    n = (mib << 20) // 4
    a = torch.rand(n, device=dev, generator=g) * 2 - 1
    b = torch.rand(n, device=dev, generator=g) * 2 - 1
    b2 = b.clone()
    torch.cuda.synchronize()
    assert L.msx_reduce_local_dev(a.data_ptr(), b.data_ptr(), n, C.MPI_FLOAT, C.MPI_SUM, sp) == 0, msx.last_error()
    assert L.msx_reduce_local_dev(a.data_ptr(), b2.data_ptr(), n, C.MPI_FLOAT, add_op, sp) == 0, msx.last_error()
    torch.cuda.synchronize()
    if not torch.equal(b.view(torch.int32), b2.view(torch.int32)):
        out["mismatches"].append(["kit add", mib])
    del b2
    # both on the SAME operands: two buffers of one size can sit differently on
    # the HBM channels, which is not what this compares
    runs = {
        "builtin_sum": lambda a=a, b=b, n=n: L.msx_reduce_local_dev(a.data_ptr(), b.data_ptr(), n, C.MPI_FLOAT,
                                                                    C.MPI_SUM, sp),
        "kit_add": lambda a=a, b=b, n=n: L.msx_reduce_local_dev(a.data_ptr(), b.data_ptr(), n, C.MPI_FLOAT,
                                                                add_op, sp),
    }
    out[f"a_combine_{mib}mib"] = measure_stream(runs, 3 * (mib << 20))
    del a, b, runs
    torch.cuda.empty_cache()

# ---- (b) MPI_Reduce_local, 64 MiB device operands: staging path against device op ----
n = (64 << 20) // 4
a = torch.randint(-2**31, 2**31 - 1, (n,), dtype=torch.int32, device=dev, generator=g)
b = {k: torch.randint(-2**31, 2**31 - 1, (n,), dtype=torch.int32, device=dev,
                      generator=torch.Generator(device=dev).manual_seed(2)) for k in ("host_twin", "device_op")}
torch.cuda.synchronize()
ops = {"host_twin": host_op("devop_nc_u32_host", 0), "device_op": device_op("devop_nc_u32", 0)}
tb = {k: {"warm": [], "cold": []} for k in ops}
def reduce_local_ms(k, op):
    t0 = time.perf_counter()
    rc = L.MPI_Reduce_local(a.data_ptr(), b[k].data_ptr(), n, C.MPI_UNSIGNED, op)
    t1 = time.perf_counter()
    assert rc == 0, msx.last_error()
    return (t1 - t0) * 1e3


for it in range(rounds):
    for k, op in ops.items():
        # warm: 2 untimed calls, then the median of 3 back to back; cold: after a flush
        reduce_local_ms(k, op); reduce_local_ms(k, op)
        tb[k]["warm"].append(sorted(reduce_local_ms(k, op) for _ in range(3))[1])
        flush_cache()
        torch.cuda.synchronize()
        tb[k]["cold"].append(reduce_local_ms(k, op))
torch.cuda.synchronize()
if not torch.equal(b["host_twin"], b["device_op"]):
    out["mismatches"].append(["reduce_local 64 MiB"])
out["b_reduce_local_64mib"] = {k: {m: summary(v) for m, v in d.items()} for k, d in tb.items()}
del a, b, flush
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
sys.exit(1 if out["mismatches"] else 0)
