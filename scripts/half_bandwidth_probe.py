"""16-bit float combines against fp32 at equal bytes per operand: MPI_SUM through
msx_reduce_local_dev (default 256 MiB per operand) and the p = 8 tree through
msx_reduce_tree_dev (default 64 MiB per source), for MPI_FLOAT, MSX_BFLOAT16 and
MSX_FLOAT16.  HIP events on one stream; the three types interleaved inside each
round; per round and type a warm figure (2 untimed calls, then 10 back to back)
and a cold one (Infinity Cache flushed by a 1 GiB read + write before each of 5
launches, median).  The fp32 spread between rounds is the yardstick a 16-bit
shortfall is held against.  Results are checked bit-exact against torch in the
same dtype first (finite inputs).  Prints one JSON line.
usage: python scripts/half_bandwidth_probe.py [combine MiB] [tree MiB] [rounds]    (GPU only)"""
import ctypes
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "microsoft-mpi_amd"))
import msx  # noqa: E402
from msx import probe  # noqa: E402

L = msx.init(errors_return=True)
C = msx.C
P = probe.lib()
comb_mib = int(sys.argv[1]) if len(sys.argv) > 1 else 256
tree_mib = int(sys.argv[2]) if len(sys.argv) > 2 else 64
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
dev = torch.device("cuda:0")
stream = torch.cuda.Stream(dev)
torch.cuda.set_stream(stream)
sp = ctypes.c_void_p(stream.cuda_stream)
flush = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
TYPES = {"fp32": (C.MPI_FLOAT, torch.float32, torch.int32), "bf16": (C.MSX_BFLOAT16, torch.bfloat16, torch.int16),
         "fp16": (C.MSX_FLOAT16, torch.float16, torch.int16)}
PEAK = 8000.0      # GB/s, the HBM figure the project's fractions use


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


def measure(runs, nbytes):
    """runs: name -> callable; nbytes: algorithmic bytes of one call."""
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
    res = {}
    for name in runs:
        w, c = sorted(warm[name]), sorted(cold[name])
        res[name] = {"warm_us": [round(x * 1e3, 1) for x in warm[name]],
                     "cold_us": [round(x * 1e3, 1) for x in cold[name]],
                     "warm_med_us": round(w[len(w) // 2] * 1e3, 1), "cold_med_us": round(c[len(c) // 2] * 1e3, 1),
                     "warm_spread": round((w[-1] - w[0]) / w[len(w) // 2], 4),
                     "cold_spread": round((c[-1] - c[0]) / c[len(c) // 2], 4),
                     "warm_frac": round(nbytes / w[len(w) // 2] / 1e6 / PEAK, 4),
                     "cold_frac": round(nbytes / c[len(c) // 2] / 1e6 / PEAK, 4)}
    return res


out = {"combine_mib": comb_mib, "tree_mib": tree_mib, "rounds": rounds, "mismatches": []}

# ---- MPI_SUM, msx_reduce_local_dev: inout (op)= in --------------------------------
nbytes = comb_mib << 20
ops, runs = {}, {}
g = torch.Generator(device=dev).manual_seed(1)
for name, (h, tdt, idt) in TYPES.items():
    n = nbytes // torch.empty(0, dtype=tdt).element_size()
    a = (torch.rand(n, device=dev, generator=g) * 2 - 1).to(tdt)
    b = (torch.rand(n, device=dev, generator=g) * 2 - 1).to(tdt)
    want = b + a
    torch.cuda.synchronize()
    assert L.msx_reduce_local_dev(a.data_ptr(), b.data_ptr(), n, h, C.MPI_SUM, sp) == 0, msx.last_error()
    torch.cuda.synchronize()
    if not torch.equal(b.view(idt), want.view(idt)):
        out["mismatches"].append(["combine", name])
    del want
    ops[name] = (a, b)
    runs[name] = (lambda a=a, b=b, n=n, h=h: L.msx_reduce_local_dev(a.data_ptr(), b.data_ptr(), n, h, C.MPI_SUM, sp))
out["combine"] = measure(runs, 3 * nbytes)
del ops, runs
torch.cuda.empty_cache()

# ---- the p = 8 tree, msx_reduce_tree_dev -------------------------------------------
nbytes = tree_mib << 20
keep, runs = [], {}
for name, (h, tdt, idt) in TYPES.items():
    n = nbytes // torch.empty(0, dtype=tdt).element_size()
    xs = [(torch.rand(n, device=dev, generator=g) * 2 - 1).to(tdt) for _ in range(8)]
    got = torch.empty(n, dtype=tdt, device=dev)
    arr = (ctypes.c_void_p * 8)(*[x.data_ptr() for x in xs])
    torch.cuda.synchronize()
    assert L.msx_reduce_tree_dev(arr, 8, got.data_ptr(), n, h, C.MPI_SUM, sp) == 0, msx.last_error()
    torch.cuda.synchronize()
    want = ((xs[0] + xs[1]) + (xs[2] + xs[3])) + ((xs[4] + xs[5]) + (xs[6] + xs[7]))
    if not torch.equal(got.view(idt), want.view(idt)):
        out["mismatches"].append(["tree", name])
    del want
    keep.append((xs, got, arr))
    runs[name] = (lambda arr=arr, got=got, n=n, h=h: L.msx_reduce_tree_dev(arr, 8, got.data_ptr(), n, h, C.MPI_SUM, sp))
out["tree8"] = measure(runs, 9 * nbytes)
print(json.dumps(out))
sys.exit(1 if out["mismatches"] else 0)
