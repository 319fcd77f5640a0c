"""MSX_SUM_WIDE against MPI_SUM on the same buffers: the p = 8 tree of bf16 and
fp16 sources into a ninth buffer through msx_reduce_tree_dev, at 32 MiB (the
cached form) and 64 MiB (the DRAM form) per source.  HIP events on one stream;
the two ops interleaved inside each of 5 rounds; per round and op a warm figure
(2 untimed calls, then 10 back to back) and a cold one (Infinity Cache flushed
by a 1 GiB read + write before each of 5 launches, median).  The yardstick is
MPI_SUM's own tree kernel in the same process: its spread over the rounds is
the margin a difference is held against.  Results are checked first: MPI_SUM
against torch adding in the 16-bit type, MSX_SUM_WIDE against torch adding in
fp32 in the same association and rounding once (finite inputs).  Prints one
JSON line.
usage: python scripts/wide_tree_probe.py [MiB per source ...]                  (GPU only)
       python scripts/wide_tree_probe.py allreduce [MiB per rank] [iterations]
           one rank of an MPI_Allreduce comparison (MSX_RANK / MSX_SIZE set by
           the launcher): both ops on the same device buffers, host clock,
           median of the iterations after 3 untimed calls; prints one line."""
import ctypes
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "microsoft-mpi_amd"))
import msx  # noqa: E402

L = msx.init(errors_return=True)
C = msx.C
dev = torch.device("cuda:0")
TYPES = {"bf16": (C.MSX_BFLOAT16, torch.bfloat16), "fp16": (C.MSX_FLOAT16, torch.float16)}
OPS = {"MPI_SUM": C.MPI_SUM, "MSX_SUM_WIDE": C.MSX_SUM_WIDE}


def allreduce_rank():
    mib = int(sys.argv[2]) if len(sys.argv) > 2 else 16
    iters = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    r_, s_ = ctypes.c_int(), ctypes.c_int()
    L.MPI_Comm_rank(C.MPI_COMM_WORLD, ctypes.byref(r_))
    L.MPI_Comm_size(C.MPI_COMM_WORLD, ctypes.byref(s_))
    res = {"rank": r_.value, "p": s_.value, "mib_per_rank": mib, "iters": iters}
    g = torch.Generator(device=dev).manual_seed(10 + r_.value)
    for tname, (h, tdt) in TYPES.items():
        n = (mib << 20) // 2
        x = (torch.rand(n, device=dev, generator=g) * 2 - 1).to(tdt)
        y = torch.empty_like(x)
        torch.cuda.synchronize()
        med = {k: [] for k in OPS}
        for it in range(3 + iters):
            for oname, op in OPS.items():            # interleaved
                L.MPI_Barrier(C.MPI_COMM_WORLD)
                t0 = time.perf_counter()
                rc = L.MPI_Allreduce(x.data_ptr(), y.data_ptr(), n, h, op, C.MPI_COMM_WORLD)
                t1 = time.perf_counter()
                assert rc == 0, msx.last_error()
                if it >= 3:
                    med[oname].append(t1 - t0)
        for oname, ts in med.items():
            ts.sort()
            res[f"{tname}/{oname}"] = {"med_us": round(ts[len(ts) // 2] * 1e6, 1), "min_us": round(ts[0] * 1e6, 1),
                                       "max_us": round(ts[-1] * 1e6, 1)}
    print("rank", json.dumps(res), flush=True)
    L.MPI_Finalize()


if len(sys.argv) > 1 and sys.argv[1] == "allreduce":
    allreduce_rank()
    sys.exit(0)

from msx import probe  # noqa: E402

P = probe.lib()
sizes = [int(a) for a in sys.argv[1:]] or [32, 64]
rounds = 5
stream = torch.cuda.Stream(dev)
torch.cuda.set_stream(stream)
sp = ctypes.c_void_p(stream.cuda_stream)
flush = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
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


out = {"p": 8, "rounds": rounds, "sizes_mib": sizes, "mismatches": [], "tree8": {}}
g = torch.Generator(device=dev).manual_seed(2)
for mib in sizes:
    nbytes = mib << 20
    for tname, (h, tdt) in TYPES.items():
        n = nbytes // 2
        xs = [(torch.rand(n, device=dev, generator=g) * 2 - 1).to(tdt) for _ in range(8)]
        got = torch.empty(n, dtype=tdt, device=dev)
        arr = (ctypes.c_void_p * 8)(*[x.data_ptr() for x in xs])
        torch.cuda.synchronize()
        f = [x.float() for x in xs]
        want = {"MPI_SUM": ((xs[0] + xs[1]) + (xs[2] + xs[3])) + ((xs[4] + xs[5]) + (xs[6] + xs[7])),
                "MSX_SUM_WIDE": (((f[0] + f[1]) + (f[2] + f[3])) + ((f[4] + f[5]) + (f[6] + f[7]))).to(tdt)}
        del f
        runs = {}
        for oname, op in OPS.items():
            assert L.msx_reduce_tree_dev(arr, 8, got.data_ptr(), n, h, op, sp) == 0, msx.last_error()
            torch.cuda.synchronize()
            if not torch.equal(got.view(torch.int16), want[oname].view(torch.int16)):
                out["mismatches"].append([mib, tname, oname])
            runs[oname] = (lambda op=op: L.msx_reduce_tree_dev(arr, 8, got.data_ptr(), n, h, op, sp))
        out["differ_frac"] = out.get("differ_frac", {})
        out["differ_frac"][f"{mib}/{tname}"] = round(
            float((want["MPI_SUM"].view(torch.int16) != want["MSX_SUM_WIDE"].view(torch.int16)).float().mean()), 4)
        del want
        out["tree8"][f"{mib}MiB/{tname}"] = measure(runs, 9 * nbytes)
        del xs, got, runs
        torch.cuda.empty_cache()
print(json.dumps(out))
sys.exit(1 if out["mismatches"] else 0)
