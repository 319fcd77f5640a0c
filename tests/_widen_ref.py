"""numpy definition of msx_accumulate_widen_dev (include/msx.h): a 16-bit float
origin combined into an fp32 target.  Nothing here comes from the library.

  W(x)  widens a uint16 bit pattern to the uint32 pattern of the same value,
        stated in integers: bf16 is x << 16; fp16 is exact for every non-NaN
        pattern (subnormals normalised by hand) and a NaN keeps sign, payload
        and signalling state: sign << 31 | 0x7F800000 | m << 13.  No astype:
        numpy's and torch's fp16 -> fp32 conversions disagree on signalling
        NaNs.
  combine(op, dt, origin, target): oracle.reduce_local(op, MPI_FLOAT,
        W(origin), target), the oracle's fp32 restatement of op.cpp, the
        target in the `inout` role; MPI_REPLACE is W(origin).
"""
import numpy as np

import msx
import oracle
import _half_ref as R

TYPES = R.TYPES
OPS = ("MPI_SUM", "MPI_PROD", "MPI_MAX", "MPI_MIN", "MPI_REPLACE")


def w_bf16(x):
    return np.ascontiguousarray(x, dtype=np.uint16).astype(np.uint32) << 16


def w_f16(x):
    x = np.ascontiguousarray(x, dtype=np.uint16).astype(np.uint32)
    sign, e, m = (x & 0x8000) << 16, (x >> 10) & 0x1F, x & 0x3FF
    normal = sign | ((e + 112) << 23) | (m << 13)
    special = sign | 0x7F800000 | (m << 13)                  # inf (m == 0) and every NaN
    # a subnormal is m * 2^-24: shift the leading one of m up to bit 10
    lead = np.zeros_like(m)
    for b in range(10):
        lead[(m >> b) > 0] = b                               # position of the leading one
    sh = 10 - lead
    sub = sign | ((113 - sh) << 23) | (((m << sh) & 0x3FF) << 13)
    out = np.where(e == 31, special, np.where(e == 0, np.where(m == 0, sign, sub), normal))
    return out.astype(np.uint32)


W = {"MSX_FLOAT16": w_f16, "MSX_BFLOAT16": w_bf16}


def is_nan16(dt, x):
    x = np.ascontiguousarray(x, dtype=np.uint16)
    inf = 0x7C00 if dt == "MSX_FLOAT16" else 0x7F80
    return (x & 0x7FFF) > inf


def combine(op, dt, origin, target):
    """New target (uint32 patterns) of `target (op)= W(origin)`; origin uint16
    patterns, target uint32 patterns of the same length."""
    w = W[dt](origin)
    if op == "MPI_REPLACE":
        return w
    exp = np.ascontiguousarray(target, dtype=np.uint32).copy().view(np.float32)
    if exp.size:
        assert oracle.reduce_local(getattr(msx.C, op), msx.C.MPI_FLOAT, w.view(np.float32), exp) == 0
    return exp.view(np.uint32)


def self_test():
    """W against _half_ref on every non-NaN pattern, and the round trip."""
    x = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)
    for dt in TYPES:
        ok = ~is_nan16(dt, x)
        w = W[dt](x)
        assert np.array_equal(w[ok], R.W[dt](x[ok]).view(np.uint32)), dt
        assert np.array_equal(R.N[dt](w[ok].view(np.float32)), x[ok]), dt
        assert np.unique(w).size == 1 << 16, dt                       # injective, NaNs included
    # the fp16 NaN rule, spelled out on three patterns
    assert [hex(v) for v in w_f16(np.array([0x7C01, 0xFE00, 0x7DFF], np.uint16))] == \
        ["0x7f802000", "0xffc00000", "0x7fbfe000"]
