"""The DRAM-regime combine (k_combine_dram) above its tile permutation, and the
probe library's cache-policy variants of its body.

The XCD-run tile order only permutes anything above 1024 one-wave workgroups
(8 XCDs x runs of 128 tiles); test_dram_regime_kernel_every_pair stays below
that for 1-8-byte types.  Here every element size runs 1024*64 + 3*64 + 5
sixteen-byte vectors plus a ragged tail: 1024 permuted tiles, three full tiles
in dispatch order behind them, one partial tile, scalar head and tail.  Bit
exact against the oracle, no tolerance: one operation per element.

Every case also runs twice in a row on the same `inout` (aligned operands for
the product, all variants of the probe library): a store policy that left
stale lines where the next launch's loads find them would show in the second
result.
"""
import ctypes
import os
import subprocess
import sys

import pytest

import msx

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NVEC = 1024 * 64 + 3 * 64 + 5

_CHILD = r'''
import ctypes, os, sys, zlib
sys.path.insert(0, os.path.join(REPO, "microsoft-mpi_amd")); sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np, torch
import msx, oracle
from _cases import KIND, gen, h
L = msx.init(errors_return=True)
s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
bad, ran = [], 0

def dev(x, off):
    raw = np.frombuffer(x.tobytes(), np.uint8)
    t = torch.zeros(raw.size + off + 64, dtype=torch.uint8, device="cuda")
    t[off:off + raw.size] = torch.from_numpy(raw.copy()).cuda()
    return t

for op, dt in PAIRS:
    assert oracle.op_check(h(op), h(dt)) == 0, (op, dt)
    rng = np.random.default_rng(zlib.crc32(f"policy/{op}/{dt}".encode()))
    a0 = gen(KIND[dt], op, 1, rng)
    es = a0.dtype.itemsize
    epv = 16 // es
    n = NVEC * epv + (epv - 1 if epv > 1 else 0)          # ragged tail where the type has one
    for off in (0, es):                                   # both 16-byte aligned / both one element on
        a = np.frombuffer(bytearray(gen(KIND[dt], op, n, rng).tobytes()), dtype=a0.dtype)
        b = np.frombuffer(bytearray(gen(KIND[dt], op, n, rng).tobytes()), dtype=a0.dtype)
        exp = [np.frombuffer(bytearray(b.tobytes()), dtype=a.dtype)]
        assert oracle.reduce_local(h(op), h(dt), a, exp[0]) == 0
        if off == 0:                                      # a second launch on the same inout
            exp.append(np.frombuffer(bytearray(exp[0].tobytes()), dtype=a.dtype))
            assert oracle.reduce_local(h(op), h(dt), a, exp[1]) == 0
        ta, tb = dev(a, off), dev(b, off)
        assert (ta.data_ptr() + off) % 16 == off % 16 and (tb.data_ptr() + off) % 16 == off % 16
        torch.cuda.synchronize()
        for k, e in enumerate(exp):
            rc = L.msx_reduce_local_dev(ta.data_ptr() + off, tb.data_ptr() + off, n, h(dt), h(op), s)
            torch.cuda.synchronize()
            got = tb[off:off + b.nbytes].cpu().numpy().tobytes()
            ran += 1
            if rc or got != e.tobytes():
                bad.append(f"{op} {dt} n={n} off={off} launch={k} rc={rc}")
        guard = tb.cpu().numpy()
        if guard[:off].any() or guard[off + b.nbytes:].any():
            bad.append(f"{op} {dt} off={off}: bytes outside inout written")
print("POLICY_BAD", len(bad), ran, bad[:6], flush=True)
'''

# one op per element size (1, 2, 4, 8, 16 bytes) and one bitwise op on bytes
PAIRS = [("MPI_SUM", "MPI_INT8_T"), ("MPI_PROD", "MPI_INT16_T"), ("MPI_SUM", "MPI_FLOAT"),
         ("MPI_MAX", "MPI_DOUBLE"), ("MPI_PROD", "MPI_C_DOUBLE_COMPLEX"), ("MPI_BXOR", "MPI_BYTE")]


def test_dram_kernel_above_the_tile_permutation():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    env = dict(os.environ, MSX_TEST_COMBINE_DRAM_MIN="0")
    head = f"REPO={msx.REPO_ROOT!r}\nNVEC={NVEC}\nPAIRS={PAIRS!r}\n"
    r = subprocess.run([sys.executable, "-c", head + _CHILD], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("POLICY_BAD")]
    assert line, (r.stdout + r.stderr)[-3000:]
    f = line[0].split()
    # 6 pairs x (2 launches aligned + 1 offset)
    assert f[1] == "0" and f[2] == str(3 * len(PAIRS)), (r.stdout + r.stderr)[-3000:]


def test_probe_variants_bit_exact_twice():
    """Every variant of the probe library (launch geometries and the per-stream
    cache policies) on 262144 + 1027 fp32 starting one element past 16-byte
    alignment: 1028 one-wave tiles, head of 3 and a ragged tail; twice in a
    row on the same buffers, against torch's fp32 add."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from msx import probe
    P = probe.lib()
    names = probe.variants()
    pol = [f"in_{i}_io_{o}_st_{s}" for i in ("plain", "nt", "sc1", "sc1nt") for o in ("plain", "nt")
           for s in ("plain", "nt", "sc1", "sc0sc1")]
    assert "default_body_probe" in names and not [p for p in pol if p not in names]
    n = 262144 + 1027
    g = torch.Generator(device="cuda").manual_seed(0xC0FFEE)
    src = torch.rand(n + 1, device="cuda", generator=g) * 2 - 1
    acc = torch.rand(n + 1, device="cuda", generator=g) * 2 - 1
    assert src.data_ptr() % 16 == 0 and acc.data_ptr() % 16 == 0
    once = acc + src
    twice = once + src
    once[0] = twice[0] = acc[0]                # element 0 lies before the operand
    sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    bad = []
    for name, v in names.items():
        c = acc.clone()
        torch.cuda.synchronize()
        for want in (once, twice):
            rc = P.msxp_variant_run(v, src.data_ptr() + 4, c.data_ptr() + 4, n, sp)
            torch.cuda.synchronize()
            if rc or not torch.equal(c.view(torch.int32), want.view(torch.int32)):
                bad.append(name)
                break
    assert not bad, bad
