"""msx_reduce_local_batch_dev against the launches it replaces, on one MI355X.

fp32 MPI_SUM, finite inputs.  256 segments, consecutive slices of one buffer
per operand, at 64 KiB per segment (16 MiB per operand in all) and again at
4 KiB (1 MiB in all).  The candidates run on the SAME buffers in the same
process, interleaved inside each of 5 rounds, HIP events on one stream; per
round a warm figure (2 untimed runs, then 10 back to back) and a cold one
(Infinity Cache flushed by a 1 GiB read + write before each of 5 runs, median).
Each figure's spread over the rounds is recorded beside it.
  a_batch       the 256 segments through ONE msx_reduce_local_batch_dev call
  b_per_segment the same segments through 256 msx_reduce_local_dev calls, what
                the batch call replaces (driven through ctypes like a_batch;
                the cost of 256 empty ctypes calls is recorded as ctypes_us)
  c_contiguous  one msx_reduce_local_dev over the whole buffer: the floor for
                those bytes
  d             one segment both ways, msx_reduce_local_batch_dev against
                msx_reduce_local_dev: 256 MiB with the 64 KiB set (the same
                launch by construction), one 4 KiB segment with the 4 KiB set
                (k_combine_segs against k_combine)
Gate (64 KiB set): a_batch is faster than b_per_segment, warm and cold, by more
than the sum of the two spreads.  a / c and d are recorded, not gated.
The batch's bytes are compared with the per-segment calls' first.  Prints one
JSON line; --out FILE also writes it there.
usage: python scripts/batch_combine_probe.py [--out FILE] [--rounds N]    (GPU only)"""
import ctypes
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "microsoft-mpi_amd"))

import torch  # noqa: E402

import msx  # noqa: E402
from msx import probe  # noqa: E402

rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 5
L = msx.init(errors_return=True)
C = msx.C
assert torch.cuda.is_available() and L.msx_device_count() > 0, "the probe needs an MI355X"
P = probe.lib()
dev = torch.device("cuda:0")
stream = torch.cuda.Stream(dev)
torch.cuda.set_stream(stream)
sp = ctypes.c_void_p(stream.cuda_stream)
flush = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
NSEG = 256


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


def summary(ts, nbytes):
    s = sorted(ts)
    med = s[len(s) // 2]
    return {"us": [round(x * 1e3, 2) for x in ts], "med_us": round(med * 1e3, 2),
            "spread": round((s[-1] - s[0]) / med, 4), "gbs": round(nbytes / med / 1e6, 1)}


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
    return {k: {"warm": summary(warm[k], nbytes[k]), "cold": summary(cold[k], nbytes[k])} for k in runs}


def over(m, num, den, mode):
    return round(m[num][mode]["med_us"] / m[den][mode]["med_us"], 3)


out = {"rounds": rounds, "nseg": NSEG, "mismatches": [], "gate_ok": True}
g = torch.Generator(device=dev).manual_seed(1)

# the cost of the 256 ctypes calls themselves (count == 0 returns at once)
t0 = time.perf_counter()
for _ in range(10 * NSEG):
    L.msx_reduce_local_dev(None, None, 0, C.MPI_FLOAT, C.MPI_SUM, sp)
out["ctypes_us"] = round((time.perf_counter() - t0) / 10 * 1e6, 1)

for seg_kib in (64, 4):
    seg_el = (seg_kib << 10) // 4
    n = NSEG * seg_el
    a = torch.rand(n, device=dev, generator=g) * 2 - 1
    b = torch.rand(n, device=dev, generator=g) * 2 - 1
    pa = [a.data_ptr() + 4 * seg_el * k for k in range(NSEG)]
    pb = [b.data_ptr() + 4 * seg_el * k for k in range(NSEG)]
    A, B = (ctypes.c_void_p * NSEG)(*pa), (ctypes.c_void_p * NSEG)(*pb)
    N = (ctypes.c_int64 * NSEG)(*[seg_el] * NSEG)
    plan = [ctypes.c_int() for _ in range(4)]
    assert L.msx_reduce_local_batch_plan(A, B, N, NSEG, C.MPI_FLOAT, C.MPI_SUM, *[ctypes.byref(x) for x in plan]) == 0

    def a_batch(A=A, B=B, N=N):
        return L.msx_reduce_local_batch_dev(A, B, N, NSEG, C.MPI_FLOAT, C.MPI_SUM, sp)

    def b_per_segment(pa=pa, pb=pb, seg_el=seg_el):
        rc = 0
        for x, y in zip(pa, pb):
            rc |= L.msx_reduce_local_dev(x, y, seg_el, C.MPI_FLOAT, C.MPI_SUM, sp)
        return rc

    def c_contiguous(a=a, b=b, n=n):
        return L.msx_reduce_local_dev(a.data_ptr(), b.data_ptr(), n, C.MPI_FLOAT, C.MPI_SUM, sp)

    # the same bytes first
    b0 = b.clone()
    torch.cuda.synchronize()
    assert a_batch() == 0, msx.last_error()
    got = b.clone()
    b.copy_(b0)
    assert b_per_segment() == 0, msx.last_error()
    torch.cuda.synchronize()
    if not torch.equal(got.view(torch.int32), b.view(torch.int32)):
        out["mismatches"].append(["batch against per-segment calls", seg_kib])
    b.copy_(b0)                    # a few hundred timed repetitions of b += a stay finite
    torch.cuda.synchronize()

    runs = {"a_batch": a_batch, "b_per_segment": b_per_segment, "c_contiguous": c_contiguous}
    m = measure(runs, {k: 3 * 4 * n for k in runs})
    m["plan"] = dict(zip(("width", "launches", "batched", "single"), (x.value for x in plan)))
    for mode in ("warm", "cold"):
        m[f"{mode}_b_over_a"] = over(m, "b_per_segment", "a_batch", mode)
        m[f"{mode}_a_over_c"] = over(m, "a_batch", "c_contiguous", mode)
        ok = m[f"{mode}_b_over_a"] - 1 > m["a_batch"][mode]["spread"] + m["b_per_segment"][mode]["spread"]
        m[f"{mode}_a_faster_beyond_spreads"] = bool(ok)
        if seg_kib == 64:
            out["gate_ok"] = out["gate_ok"] and bool(ok)
    out[f"segments_{seg_kib}kib"] = m
    del a, b, b0, got, runs
    torch.cuda.empty_cache()

    # d: one segment both ways
    n1 = (256 << 20) // 4 if seg_kib == 64 else seg_el
    a = torch.rand(n1, device=dev, generator=g) * 2 - 1
    b = torch.rand(n1, device=dev, generator=g) * 1e-3
    A1, B1, N1 = (ctypes.c_void_p * 1)(a.data_ptr()), (ctypes.c_void_p * 1)(b.data_ptr()), (ctypes.c_int64 * 1)(n1)

    def d_batch(A1=A1, B1=B1, N1=N1):
        return L.msx_reduce_local_batch_dev(A1, B1, N1, 1, C.MPI_FLOAT, C.MPI_SUM, sp)

    def d_direct(a=a, b=b, n1=n1):
        return L.msx_reduce_local_dev(a.data_ptr(), b.data_ptr(), n1, C.MPI_FLOAT, C.MPI_SUM, sp)

    torch.cuda.synchronize()
    assert d_batch() == 0 and d_direct() == 0, msx.last_error()
    runs = {"d_batch": d_batch, "d_direct": d_direct}
    m = measure(runs, {k: 3 * 4 * n1 for k in runs})
    for mode in ("warm", "cold"):
        r = over(m, "d_batch", "d_direct", mode)
        m[f"{mode}_batch_over_direct"] = r
        m[f"{mode}_within_direct_spread"] = bool(abs(r - 1) <= m["d_direct"][mode]["spread"])
    out[f"d_one_segment_{'256mib' if seg_kib == 64 else '4kib'}"] = m
    del a, b, runs
    torch.cuda.empty_cache()

text = json.dumps(out)
print(text)
if "--out" in sys.argv:
    path = sys.argv[sys.argv.index("--out") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
sys.exit(1 if out["mismatches"] or not out["gate_ok"] else 0)
