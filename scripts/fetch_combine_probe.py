"""msx_fetch_and_op_dev / msx_get_accumulate_dev against the two calls each
replaces, and the cache policy of the `fetched` store, on one MI355X.

fp32 MPI_SUM, finite inputs, three buffers of 256 MiB (in / origin, fetched /
result, inout / target).  The candidates of one part run on the SAME buffers in
the same process, interleaved inside each of 5 rounds, HIP events on one stream;
per round a warm figure (2 untimed runs, then 10 back to back) and a cold one
(Infinity Cache flushed by a 1 GiB read + write before each of 5 runs, median).
Each figure's spread over the rounds is recorded beside it.

contiguous_256MiB   64 Mi fp32 per operand, the DRAM-regime kernel
  a_fused            ONE msx_fetch_and_op_dev (k_fetch_combine_dram)
  b_sequence         msx_copy_dev(inout -> fetched), msx_reduce_local_dev: what a
                     caller had before
  default_fetch_probe, fetched_st_plain / _nt / _sc1 / _sc0sc1
                     the probe library's copies of the fused kernel: the
                     product's body under another symbol, and the same body with
                     each cache policy on the store of `fetched`
subarray3d_rows1536B  the 3-D C-order subarray (192, 400, 384) of (256, 512, 512)
                     at (32, 56, 64), the same datatype on all three sides
  a_fused            ONE msx_get_accumulate_dev (the three-layout kernel; the
                     plan says so)
  b_sequence         msx_accumulate_dev(MPI_REPLACE, target -> result), then
                     msx_accumulate_dev(MPI_SUM, origin -> target)
By bytes a moves 4 N and b 5 N (N = the data bytes).  Nothing is gated on a
ratio: the figures are recorded.  Every candidate's two outputs are compared
byte for byte with b_sequence's first; a mismatch is the only failure.
Prints one JSON line; --out FILE also writes it there.
usage: python scripts/fetch_combine_probe.py [--out FILE] [--rounds N]    (GPU only)"""
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


out = {"rounds": rounds, "span_mib": 256, "mismatches": []}
g = torch.Generator(device=dev).manual_seed(1)
nf = 256 << 18                                                     # fp32 elements in 256 MiB
origin = torch.rand(nf, device=dev, generator=g) * 2 - 1
target = torch.rand(nf, device=dev, generator=g) * 1e-3
result = torch.zeros(nf, dtype=torch.float32, device=dev)
t0 = target.clone()


def same_as_sequence(runs, part):
    """Every candidate's target and result against b_sequence's, byte for byte."""
    target.copy_(t0); result.zero_()
    torch.cuda.synchronize()
    assert runs["b_sequence"]() == 0, msx.last_error()
    torch.cuda.synchronize()
    want_t, want_r = target.clone(), result.clone()
    assert not torch.equal(want_t, t0) and not torch.equal(want_r, torch.zeros_like(want_r))
    for k, fn in runs.items():
        if k == "b_sequence":
            continue
        target.copy_(t0); result.zero_()
        torch.cuda.synchronize()
        assert fn() == 0, (k, msx.last_error())
        torch.cuda.synchronize()
        if not (torch.equal(target.view(torch.int32), want_t.view(torch.int32))
                and torch.equal(result.view(torch.int32), want_r.view(torch.int32))):
            out["mismatches"].append(f"{part}/{k}")
    target.copy_(t0)                  # a few hundred timed repetitions of target += origin stay finite
    torch.cuda.synchronize()


def ratios(m):
    for mode in ("warm", "cold"):
        a, b = m["a_fused"][mode], m["b_sequence"][mode]
        r = round(b["med_us"] / a["med_us"], 3)
        m[f"{mode}_b_over_a"] = r
        m[f"{mode}_a_frac_of_8tbs_over_4n"] = round(a["gbs"] / HBM, 4)
        m[f"{mode}_a_faster_beyond_spreads"] = bool(r - 1 > a["spread"] + b["spread"])


# ---- contiguous: msx_fetch_and_op_dev, and the `fetched` store's cache policy --------
def fetch_fused():
    return L.msx_fetch_and_op_dev(origin.data_ptr(), result.data_ptr(), target.data_ptr(), nf, C.MPI_FLOAT, C.MPI_SUM, sp)


def fetch_sequence():
    rc = L.msx_copy_dev(result.data_ptr(), target.data_ptr(), 4 * nf, sp)
    return rc | L.msx_reduce_local_dev(origin.data_ptr(), target.data_ptr(), nf, C.MPI_FLOAT, C.MPI_SUM, sp)


runs = {"a_fused": fetch_fused, "b_sequence": fetch_sequence}
for vname, v in probe.fetch_variants().items():
    runs[vname] = (lambda v=v: P.msxp_fetch_run(v, origin.data_ptr(), result.data_ptr(), target.data_ptr(), nf, sp))
same_as_sequence(runs, "contiguous_256MiB")
m = measure(runs, {k: (5 if k == "b_sequence" else 4) * 4 * nf for k in runs})
m["data_bytes"] = 4 * nf
ratios(m)
out["contiguous_256MiB"] = m

# ---- the 3-D subarray: msx_get_accumulate_dev -------------------------------------------
ia = lambda v: (ctypes.c_int * len(v))(*v)
d0 = nf // (512 * 512)
dims, sub, st = (d0, 512, 512), (d0 * 3 // 4, 400, 384), (d0 // 8, 56, 64)
t3 = ctypes.c_int()
assert L.MPI_Type_create_subarray(3, ia(dims), ia(sub), ia(st), C.MPI_ORDER_C, C.MPI_FLOAT, ctypes.byref(t3)) == 0
assert L.MPI_Type_commit(ctypes.byref(t3)) == 0
n = sub[0] * sub[1] * sub[2]
el, path, gran = ctypes.c_int64(), ctypes.c_int(), ctypes.c_int()
assert L.msx_get_accumulate_plan(1, t3.value, 1, t3.value, 1, t3.value, C.MPI_SUM, ctypes.byref(el), ctypes.byref(path),
                                 ctypes.byref(gran)) == 0
assert (el.value, path.value, gran.value) == (n, 3, 4)


def gacc_fused():
    return L.msx_get_accumulate_dev(origin.data_ptr(), 1, t3.value, result.data_ptr(), 1, t3.value, target.data_ptr(), 1,
                                    t3.value, C.MPI_SUM, sp)


def gacc_sequence():
    rc = L.msx_accumulate_dev(target.data_ptr(), 1, t3.value, result.data_ptr(), 1, t3.value, C.MPI_REPLACE, sp)
    return rc | L.msx_accumulate_dev(origin.data_ptr(), 1, t3.value, target.data_ptr(), 1, t3.value, C.MPI_SUM, sp)


runs = {"a_fused": gacc_fused, "b_sequence": gacc_sequence}
same_as_sequence(runs, "subarray3d_rows1536B")
m = measure(runs, {"a_fused": 4 * 4 * n, "b_sequence": 5 * 4 * n})
m["data_bytes"] = 4 * n
ratios(m)
out["subarray3d_rows1536B"] = m

text = json.dumps(out)
print(text)
if "--out" in sys.argv:
    path = sys.argv[sys.argv.index("--out") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
sys.exit(1 if out["mismatches"] else 0)
