"""msx_accumulate_widen_dev (bf16 origin, fp32 target, MPI_SUM) against the fp32
combine on the same element count and against what a caller did before, on one
MI355X.

The candidates of one part run on the SAME buffers in the same process,
interleaved inside each of 5 rounds, HIP events on one stream; per round a warm
figure (2 untimed runs, then 10 back to back) and a cold one (Infinity Cache
flushed by a 1 GiB read + write before each of 5 runs, median).  Each figure's
spread over the rounds is recorded beside it.

contiguous_64Mi      64 Mi elements: 128 MiB of bf16 into 256 MiB of fp32, the
                     DRAM-regime kernel
contiguous_512Ki     512 Ki elements: 1 MiB into 2 MiB, L2-resident, the tile kernel
  a_widen            ONE msx_accumulate_widen_dev: 10 bytes per element
  b_fp32_combine     msx_reduce_local_dev, fp32 MPI_SUM, on the same element count
                     (an fp32 origin of the same values): 12 bytes per element,
                     the existing kernel, unchanged
  c_convert_combine  what a caller does today: torch's .float() of the origin
                     into a scratch tensor (copy_), then b: 18 bytes per element
subarray3d           the bf16 C-order subarray (192, 400, 384) of (256, 512, 512)
                     at (32, 56, 64) into the same subarray of an fp32 array
  a_widen            ONE msx_accumulate_widen_dev (the two-layout kernel; the plan
                     says so)
  b_fp32_accumulate  msx_accumulate_dev, fp32 MPI_SUM, between the two fp32
                     subarrays: 12 bytes per element
  c_pack_convert_accumulate
                     msx_pack_dev of the bf16 subarray, .float() into a scratch
                     tensor, msx_accumulate_dev from the contiguous fp32 scratch
                     into the subarray
The expectation from bytes is a <= b < c.  The criterion recorded per part and
mode: a is not slower than b by more than the spread this script records for b.
Nothing else is gated.  Every candidate's target is compared byte for byte with
a_widen's first; a mismatch is the only failure.
Prints one JSON line; --out FILE also writes it there.
usage: python scripts/widen_accumulate_probe.py [--out FILE] [--rounds N]    (GPU only)"""
import ctypes
import json
import os
import sys

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


def measure(parts):
    """parts: {part: (runs, bytes per candidate)}; every candidate of every part
    inside each round, so the sizes are interleaved too."""
    warm = {p: {k: [] for k in runs} for p, (runs, _) in parts.items()}
    cold = {p: {k: [] for k in runs} for p, (runs, _) in parts.items()}
    for _ in range(rounds):
        for p, (runs, _) in parts.items():
            for name, fn in runs.items():
                fn(); fn()
                warm[p][name].append(timed(fn, 10))
                ts = []
                for _ in range(5):
                    flush_cache()
                    ts.append(timed(fn, 1))
                cold[p][name].append(sorted(ts)[2])
    return {p: {k: {"warm": summary(warm[p][k], nb[k]), "cold": summary(cold[p][k], nb[k])} for k in runs}
            for p, (runs, nb) in parts.items()}


def verdict(m, b):
    for mode in ("warm", "cold"):
        a_us, b_us, b_spread = m["a_widen"][mode]["med_us"], m[b][mode]["med_us"], m[b][mode]["spread"]
        m[f"{mode}_a_over_b"] = round(a_us / b_us, 4)
        m[f"{mode}_a_not_slower_than_b_beyond_b_spread"] = bool(a_us <= b_us * (1 + b_spread))
        c = [k for k in m if k.startswith("c_")][0]
        m[f"{mode}_c_over_a"] = round(m[c][mode]["med_us"] / a_us, 4)


out = {"rounds": rounds, "mismatches": []}
g = torch.Generator(device=dev).manual_seed(1)


def same_targets(runs, target, t0, part):
    """Every candidate's target against a_widen's, byte for byte (the fp32
    origin holds the widened values, so all three compute the same sums)."""
    want = None
    for k, fn in runs.items():
        target.copy_(t0)
        torch.cuda.synchronize()
        assert fn() == 0, (k, msx.last_error())
        torch.cuda.synchronize()
        if want is None:
            want = target.clone()
            assert not torch.equal(want, t0)
        elif not torch.equal(target.view(torch.int32), want.view(torch.int32)):
            out["mismatches"].append(f"{part}/{k}")
    target.copy_(t0)                  # a few hundred timed repetitions of target += origin stay finite
    torch.cuda.synchronize()


def contiguous(n):
    o16 = (torch.rand(n, device=dev, generator=g) * 2 - 1).to(torch.bfloat16)
    o32 = o16.float()
    scratch = torch.empty(n, dtype=torch.float32, device=dev)
    target = torch.rand(n, device=dev, generator=g) * 1e-3
    t0 = target.clone()

    def a():
        return L.msx_accumulate_widen_dev(o16.data_ptr(), n, C.MSX_BFLOAT16, target.data_ptr(), n, C.MPI_FLOAT,
                                          C.MPI_SUM, sp)

    def b():
        return L.msx_reduce_local_dev(o32.data_ptr(), target.data_ptr(), n, C.MPI_FLOAT, C.MPI_SUM, sp)

    def c():
        scratch.copy_(o16)
        return L.msx_reduce_local_dev(scratch.data_ptr(), target.data_ptr(), n, C.MPI_FLOAT, C.MPI_SUM, sp)

    runs = {"a_widen": a, "b_fp32_combine": b, "c_convert_combine": c}
    el, path = ctypes.c_int64(), ctypes.c_int()
    assert L.msx_accumulate_widen_plan(n, C.MSX_BFLOAT16, n, C.MPI_FLOAT, C.MPI_SUM, ctypes.byref(el),
                                       ctypes.byref(path)) == 0 and (el.value, path.value) == (n, 1)
    same_targets(runs, target, t0, f"contiguous_{n}")
    return runs, {"a_widen": 10 * n, "b_fp32_combine": 12 * n, "c_convert_combine": 18 * n}, (o16, o32, scratch, target, t0)


def subarray():
    ia = lambda v: (ctypes.c_int * len(v))(*v)
    dims, sub, st = (256, 512, 512), (192, 400, 384), (32, 56, 64)
    nel = dims[0] * dims[1] * dims[2]
    n = sub[0] * sub[1] * sub[2]
    t16, t32 = ctypes.c_int(), ctypes.c_int()
    for t, base in ((t16, C.MSX_BFLOAT16), (t32, C.MPI_FLOAT)):
        assert L.MPI_Type_create_subarray(3, ia(dims), ia(sub), ia(st), C.MPI_ORDER_C, base, ctypes.byref(t)) == 0
        assert L.MPI_Type_commit(ctypes.byref(t)) == 0
    o16 = (torch.rand(nel, device=dev, generator=g) * 2 - 1).to(torch.bfloat16)
    o32 = o16.float()
    packed = torch.empty(n, dtype=torch.bfloat16, device=dev)
    scratch = torch.empty(n, dtype=torch.float32, device=dev)
    target = torch.rand(nel, device=dev, generator=g) * 1e-3
    t0 = target.clone()
    el, path = ctypes.c_int64(), ctypes.c_int()
    assert L.msx_accumulate_widen_plan(1, t16.value, 1, t32.value, C.MPI_SUM, ctypes.byref(el), ctypes.byref(path)) == 0
    assert (el.value, path.value) == (n, 2)

    def a():
        return L.msx_accumulate_widen_dev(o16.data_ptr(), 1, t16.value, target.data_ptr(), 1, t32.value, C.MPI_SUM, sp)

    def b():
        return L.msx_accumulate_dev(o32.data_ptr(), 1, t32.value, target.data_ptr(), 1, t32.value, C.MPI_SUM, sp)

    def c():
        rc = L.msx_pack_dev(o16.data_ptr(), 1, t16.value, packed.data_ptr(), sp)
        scratch.copy_(packed)
        return rc | L.msx_accumulate_dev(scratch.data_ptr(), n, C.MPI_FLOAT, target.data_ptr(), 1, t32.value, C.MPI_SUM, sp)

    runs = {"a_widen": a, "b_fp32_accumulate": b, "c_pack_convert_accumulate": c}
    same_targets(runs, target, t0, "subarray3d")
    # c: pack 2 + 2, convert 2 + 4, accumulate 4 + 4 + 4
    return runs, {"a_widen": 10 * n, "b_fp32_accumulate": 12 * n, "c_pack_convert_accumulate": 22 * n}, \
        (o16, o32, packed, scratch, target, t0), n


big, small = 64 << 20, 512 << 10
r_big, nb_big, keep_big = contiguous(big)
r_small, nb_small, keep_small = contiguous(small)
r_sub, nb_sub, keep_sub, n_sub = subarray()
m = measure({"contiguous_64Mi": (r_big, nb_big), "contiguous_512Ki": (r_small, nb_small), "subarray3d": (r_sub, nb_sub)})
for part, elements, b in (("contiguous_64Mi", big, "b_fp32_combine"), ("contiguous_512Ki", small, "b_fp32_combine"),
                          ("subarray3d", n_sub, "b_fp32_accumulate")):
    m[part]["elements"] = elements
    verdict(m[part], b)
    out[part] = m[part]

text = json.dumps(out)
print(text)
if "--out" in sys.argv:
    path = sys.argv[sys.argv.index("--out") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
sys.exit(1 if out["mismatches"] else 0)
