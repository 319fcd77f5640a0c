"""msx_accumulate_dev against the four launches it replaces, on one MI355X.

fp32 MPI_SUM, finite inputs, the same datatype on both sides, origin and target
in two buffers of 256 MiB each:
  subarray3d_rows1536B   the 3-D C-order subarray (192, 400, 384) of (256, 512,
                         512) at (32, 56, 64): whole 32-byte sectors
  vector_16B_stride32B   MPI_Type_vector(n / 8, 4, 8): half of every sector
The candidates run on the SAME buffers in the same process, interleaved inside
each of 5 rounds, HIP events on one stream; per round a warm figure (2 untimed
runs, then 10 back to back) and a cold one (Infinity Cache flushed by a 1 GiB
read + write before each of 5 runs, median).  Each figure's spread over the
rounds is recorded beside it.
  a_fused      ONE msx_accumulate_dev (the two-layout kernel; the plan says so)
  b_sequence   msx_pack_dev(origin), msx_pack_dev(target), msx_reduce_local_dev,
               msx_unpack_dev: what a caller had before, two scratch buffers
By bytes a moves 3 N and b 9 N (N = the data bytes); the measured ratios are
recorded, not gated.  a's fraction of 8 TB/s is over 3 N.
Gate (both layouts): a_fused is faster than b_sequence, warm and cold, by more
than the sum of the two spreads.  The two results are compared byte for byte
first.  Prints one JSON line; --out FILE also writes it there.
usage: python scripts/typed_combine_probe.py [--out FILE] [--rounds N]    (GPU only)"""
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "microsoft-mpi_amd"))

import torch  # noqa: E402

import msx  # noqa: E402
from msx import probe  # noqa: E402

HBM = 8000.0   # GB/s
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


def layouts(nf):
    ia = lambda v: (ctypes.c_int * len(v))(*v)
    d0 = nf // (512 * 512)
    dims, sub, st = (d0, 512, 512), (d0 * 3 // 4, 400, 384), (d0 // 8, 56, 64)
    t3, tv = ctypes.c_int(), ctypes.c_int()
    assert L.MPI_Type_create_subarray(3, ia(dims), ia(sub), ia(st), C.MPI_ORDER_C, C.MPI_FLOAT, ctypes.byref(t3)) == 0
    assert L.MPI_Type_vector(nf // 8, 4, 8, C.MPI_FLOAT, ctypes.byref(tv)) == 0
    for t in (t3, tv):
        assert L.MPI_Type_commit(ctypes.byref(t)) == 0
    return [("subarray3d_rows1536B", t3, sub[0] * sub[1] * sub[2]), ("vector_16B_stride32B", tv, nf // 2)]


out = {"rounds": rounds, "span_mib": 256, "mismatches": [], "gate_ok": True}
g = torch.Generator(device=dev).manual_seed(1)
nf = 256 << 18                                                     # fp32 elements in 256 MiB
origin = torch.rand(nf, device=dev, generator=g) * 2 - 1
target = torch.rand(nf, device=dev, generator=g) * 1e-3
t0 = target.clone()

for name, t, n in layouts(nf):
    po = torch.empty(n, dtype=torch.float32, device=dev)
    pt = torch.empty(n, dtype=torch.float32, device=dev)
    el, path, gran = ctypes.c_int64(), ctypes.c_int(), ctypes.c_int()
    assert L.msx_accumulate_plan(1, t.value, 1, t.value, C.MPI_SUM, ctypes.byref(el), ctypes.byref(path),
                                 ctypes.byref(gran)) == 0
    assert (el.value, path.value, gran.value) == (n, 4, 4)

    def a_fused(t=t):
        return L.msx_accumulate_dev(origin.data_ptr(), 1, t.value, target.data_ptr(), 1, t.value, C.MPI_SUM, sp)

    def b_sequence(t=t, n=n, po=po, pt=pt):
        rc = L.msx_pack_dev(origin.data_ptr(), 1, t.value, po.data_ptr(), sp)
        rc |= L.msx_pack_dev(target.data_ptr(), 1, t.value, pt.data_ptr(), sp)
        rc |= L.msx_reduce_local_dev(po.data_ptr(), pt.data_ptr(), n, C.MPI_FLOAT, C.MPI_SUM, sp)
        return rc | L.msx_unpack_dev(pt.data_ptr(), 1, t.value, target.data_ptr(), sp)

    # the same bytes first
    torch.cuda.synchronize()
    assert a_fused() == 0, msx.last_error()
    got = target.clone()
    target.copy_(t0)
    assert b_sequence() == 0, msx.last_error()
    torch.cuda.synchronize()
    if not torch.equal(got.view(torch.int32), target.view(torch.int32)) or torch.equal(got, t0):
        out["mismatches"].append(name)
    target.copy_(t0)                  # a few hundred timed repetitions of target += origin stay finite
    del got
    torch.cuda.synchronize()

    runs = {"a_fused": a_fused, "b_sequence": b_sequence}
    m = measure(runs, {"a_fused": 3 * 4 * n, "b_sequence": 9 * 4 * n})
    m["data_bytes"] = 4 * n
    for mode in ("warm", "cold"):
        r = round(m["b_sequence"][mode]["med_us"] / m["a_fused"][mode]["med_us"], 3)
        m[f"{mode}_b_over_a"] = r
        m[f"{mode}_a_frac_of_8tbs_over_3n"] = round(m["a_fused"][mode]["gbs"] / HBM, 4)
        ok = r - 1 > m["a_fused"][mode]["spread"] + m["b_sequence"][mode]["spread"]
        m[f"{mode}_a_faster_beyond_spreads"] = bool(ok)
        out["gate_ok"] = out["gate_ok"] and bool(ok)
    out[name] = m
    target.copy_(t0)
    del po, pt, runs
    torch.cuda.empty_cache()

text = json.dumps(out)
print(text)
if "--out" in sys.argv:
    path = sys.argv[sys.argv.index("--out") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
sys.exit(1 if out["mismatches"] or not out["gate_ok"] else 0)
