"""msx_accumulate_batch_dev against the launches it replaces, on one MI355X.

fp32 MPI_SUM, finite inputs.  The candidates run on the SAME buffers in the same
process, interleaved inside each of 5 rounds, HIP events on one stream; per
round a warm figure (2 untimed runs, then 10 back to back) and a cold one
(Infinity Cache flushed by a 1 GiB read + write before each of 5 runs, median).
Each figure's spread over the rounds is recorded beside it.
  a_batch       the segments through ONE msx_accumulate_batch_dev call
  b_per_segment the same segments through one msx_accumulate_dev each, what the
                batch call replaces (driven through ctypes like a_batch; the
                cost of as many empty ctypes calls is recorded as ctypes_us)
Workloads:
  halo_buffers  six disjoint one-cell faces of a 256^3 block (x whole, y without
                the x edges, z without both) summed from six contiguous receive
                buffers: the halo sum
  halo_faces    the same faces summed from the faces of a second array
  pieces26      the 26 neighbour pieces (faces, edges, corners) of a 64^3 block
                from 26 contiguous buffers
  twelve_*      twelve equal segments at 1, 4 and 16 MiB each, contiguous on
                both sides and as a 3-D subarray (256-float rows of a 96 x 384
                plane) on both sides: the fuse_below decision.  A segment of
                exactly fuse_below bytes is launched on its own, so every
                segment is one 64-row plane (64 KiB) short of its size and the
                size at the limit is still fused; each row's plan says what
                ran.  (The decision itself was measured with the limit at its
                first value, 16 MiB: profiles/typed/typed_batch_limit16.json.)
Gate (halo_buffers): a_batch is faster than b_per_segment, warm and cold, by
more than the sum of the two spreads.  The others are recorded, not gated.
The batch's bytes are compared with the per-segment calls' first.  Prints one
JSON line; --out FILE also writes it there.
usage: python scripts/typed_batch_probe.py [--out FILE] [--rounds N]    (GPU only)"""
import ctypes
import itertools
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
vp, i64, c_int = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
F = C.MPI_FLOAT
types = []


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
    return {k: {"warm": summary(warm[k], nbytes), "cold": summary(cold[k], nbytes)} for k in runs}


def subarray(sizes, sub, start):
    n = len(sizes)
    arr = lambda v: (c_int * n)(*v)
    out = c_int()
    assert L.MPI_Type_create_subarray(n, arr(sizes), arr(sub), arr(start), C.MPI_ORDER_C, F, ctypes.byref(out)) == 0
    assert L.MPI_Type_commit(ctypes.byref(out)) == 0
    types.append(out.value)
    return out.value


def rand(n, g, scale=1.0):
    return (torch.rand(n, device=dev, generator=g) * 2 - 1) * scale


def workload(name, segs, targets, gate):
    """segs: (origin address, origin count, origin type, target address, target
    count, target type, data bytes); targets: the tensors the segments write."""
    n = len(segs)
    A = [(vp * n)(*[s[0] for s in segs]), (i64 * n)(*[s[1] for s in segs]), (c_int * n)(*[s[2] for s in segs]),
         (vp * n)(*[s[3] for s in segs]), (i64 * n)(*[s[4] for s in segs]), (c_int * n)(*[s[5] for s in segs])]
    plan = [c_int(), i64(), c_int(), c_int(), c_int()]
    assert L.msx_accumulate_batch_plan(A[1], A[2], A[4], A[5], n, C.MPI_SUM, *[ctypes.byref(x) for x in plan]) == 0

    def a_batch():
        return L.msx_accumulate_batch_dev(*A, n, C.MPI_SUM, sp)

    def b_per_segment():
        rc = 0
        for s in segs:
            rc |= L.msx_accumulate_dev(s[0], s[1], s[2], s[3], s[4], s[5], C.MPI_SUM, sp)
        return rc

    # the same bytes first
    before = [t.clone() for t in targets]
    torch.cuda.synchronize()
    assert a_batch() == 0, msx.last_error()
    got = [t.clone() for t in targets]
    for t, b in zip(targets, before):
        t.copy_(b)
    assert b_per_segment() == 0, msx.last_error()
    torch.cuda.synchronize()
    for t, x, b in zip(targets, got, before):
        if not torch.equal(x.view(torch.int32), t.view(torch.int32)) or torch.equal(x.view(torch.int32), b.view(torch.int32)):
            out["mismatches"].append(name)
        t.copy_(b)                 # a few hundred timed repetitions of target += origin stay finite
    torch.cuda.synchronize()
    # the cost of the n ctypes calls themselves (no origin data bytes returns at once)
    t0 = time.perf_counter()
    for _ in range(10 * n):
        L.msx_accumulate_dev(None, 0, F, None, 0, F, C.MPI_SUM, sp)
    ctypes_us = round((time.perf_counter() - t0) / 10 * 1e6, 1)
    nbytes = 3 * sum(s[6] for s in segs)
    m = measure({"a_batch": a_batch, "b_per_segment": b_per_segment}, nbytes)
    m["ctypes_us"] = ctypes_us
    m["nseg"], m["bytes_per_segment"] = n, [s[6] for s in segs] if len({s[6] for s in segs}) > 1 else segs[0][6]
    m["plan"] = dict(zip(("width", "fuse_below", "launches", "batched", "single"), (x.value for x in plan)))
    for mode in ("warm", "cold"):
        r = round(m["b_per_segment"][mode]["med_us"] / m["a_batch"][mode]["med_us"], 3)
        m[f"{mode}_b_over_a"] = r
        ok = r - 1 > m["a_batch"][mode]["spread"] + m["b_per_segment"][mode]["spread"]
        m[f"{mode}_a_faster_beyond_spreads"] = bool(ok)
        if gate:
            out["gate_ok"] = out["gate_ok"] and bool(ok)
    out[name] = m


def faces(n):
    return [((1, n, n), (0, 0, 0)), ((1, n, n), (n - 1, 0, 0)), ((n - 2, 1, n), (1, 0, 0)), ((n - 2, 1, n), (1, n - 1, 0)),
            ((n - 2, n - 2, 1), (1, 1, 0)), ((n - 2, n - 2, 1), (1, 1, n - 1))]


def prod(v):
    return v[0] * v[1] * v[2]


out = {"rounds": rounds, "mismatches": [], "gate_ok": True}
g = torch.Generator(device=dev).manual_seed(1)

# ---- the halo sum of a 256^3 block ------------------------------------------------------
N = 256
block, second = rand(N ** 3, g, 1e-3), rand(N ** 3, g)
ftypes = [subarray((N, N, N), sub, start) for sub, start in faces(N)]
bufs = [rand(prod(sub), g) for sub, _ in faces(N)]
workload("halo_buffers", [(b.data_ptr(), b.numel(), F, block.data_ptr(), 1, t, 4 * b.numel()) for b, t in zip(bufs, ftypes)],
         [block], gate=True)
workload("halo_faces", [(second.data_ptr(), 1, t, block.data_ptr(), 1, t, 4 * b.numel()) for b, t in zip(bufs, ftypes)],
         [block], gate=False)
del block, second, bufs
torch.cuda.empty_cache()

# ---- the 26 neighbour pieces of a 64^3 block ------------------------------------------
N = 64
block = rand(N ** 3, g, 1e-3)
cut = {-1: (0, 1), 0: (1, N - 2), 1: (N - 1, 1)}          # (start, size) along one axis
segs = []
keepalive = []
for d in itertools.product((-1, 0, 1), repeat=3):
    if d == (0, 0, 0):
        continue
    start, sub = tuple(cut[x][0] for x in d), tuple(cut[x][1] for x in d)
    b = rand(prod(sub), g)
    keepalive.append(b)
    segs.append((b.data_ptr(), b.numel(), F, block.data_ptr(), 1, subarray((N, N, N), sub, start), 4 * b.numel()))
workload("pieces26", segs, [block], gate=False)
del block, keepalive
torch.cuda.empty_cache()

# ---- twelve equal segments: where fusing stops paying -----------------------------------
NSEG, ROW, PLANE = 12, 256, (96, 384)
for mib in (1, 4, 16):
    rows = (mib << 20) // (4 * ROW) - 64                   # one 64-row plane short of the size
    n = rows * ROW
    a, b = rand(NSEG * n, g), rand(NSEG * n, g, 1e-3)
    workload(f"twelve_contiguous_{mib}mib",
             [(a.data_ptr() + 4 * n * k, n, F, b.data_ptr() + 4 * n * k, n, F, 4 * n) for k in range(NSEG)], [b], gate=False)
    del a, b
    planes = rows // 64                                    # 64 rows of each 96-row plane
    assert planes * 64 == rows
    t = subarray((planes,) + PLANE, (planes, 64, ROW), (0, 16, 64))
    span = planes * PLANE[0] * PLANE[1]
    a, b = rand(NSEG * span, g), rand(NSEG * span, g, 1e-3)
    workload(f"twelve_subarray_{mib}mib",
             [(a.data_ptr() + 4 * span * k, 1, t, b.data_ptr() + 4 * span * k, 1, t, 4 * n) for k in range(NSEG)], [b],
             gate=False)
    del a, b
    torch.cuda.empty_cache()

for t in reversed(types):
    x = c_int(t)
    L.MPI_Type_free(ctypes.byref(x))
text = json.dumps(out)
print(text)
if "--out" in sys.argv:
    path = sys.argv[sys.argv.index("--out") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
sys.exit(1 if out["mismatches"] or not out["gate_ok"] else 0)
