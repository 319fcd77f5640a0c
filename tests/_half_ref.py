"""numpy definition of the 16-bit float combines (MSX_FLOAT16, MSX_BFLOAT16).

This is the definition the kernels are held to, bit for bit; nothing here
comes from the library.  Operands and results are uint16 bit patterns.

  w(x)  widens exactly to fp32, n(r) rounds an fp32 to the 16-bit format
        (nearest-even, subnormals, overflow to +-inf);
  SUM / PROD: r = w(inout) op w(in), one IEEE fp32 operation; n(r) unless r is
        a NaN, then the x86 rule in the narrow format, inout first: inout's
        bits quieted if inout is a NaN, else in's bits quieted, else the
        sign-set default NaN;
  MAX / MIN: w(inout) > w(in) ? inout : in  ('<' for MIN), bits unchanged.
"""
import numpy as np

TYPES = ("MSX_FLOAT16", "MSX_BFLOAT16")
OPS = ("MPI_SUM", "MPI_PROD", "MPI_MAX", "MPI_MIN")
QBIT = {"MSX_FLOAT16": 0x0200, "MSX_BFLOAT16": 0x0040}
DNAN = {"MSX_FLOAT16": 0xFE00, "MSX_BFLOAT16": 0xFFC0}


def w_bf16(u):
    return (u.astype(np.uint32) << 16).view(np.float32)


def n_bf16(f):
    x = f.view(np.uint32).astype(np.uint64)
    return ((x + 0x7FFF + ((x >> 16) & 1)) >> 16).astype(np.uint16)


def w_f16(u):
    return u.view(np.float16).astype(np.float32)


def n_f16(f):
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return f.astype(np.float16).view(np.uint16)


W = {"MSX_FLOAT16": w_f16, "MSX_BFLOAT16": w_bf16}
N = {"MSX_FLOAT16": n_f16, "MSX_BFLOAT16": n_bf16}


def combine(op, dt, inout, in_):
    """New inout (uint16 array) of `inout (op)= in`."""
    io = np.ascontiguousarray(inout, dtype=np.uint16)
    x = np.ascontiguousarray(in_, dtype=np.uint16)
    a, b = W[dt](io), W[dt](x)
    with np.errstate(all="ignore"):
        if op == "MPI_MAX":
            return np.where(a > b, io, x).astype(np.uint16)
        if op == "MPI_MIN":
            return np.where(a < b, io, x).astype(np.uint16)
        if op == "MPI_SUM":
            r = a + b
        elif op == "MPI_PROD":
            r = a * b
        else:
            raise ValueError(op)
    assert r.dtype == np.float32
    rnan = np.isnan(r)
    out = N[dt](np.where(rnan, np.float32(0), r).astype(np.float32))
    q = np.uint16(QBIT[dt])
    nan_out = np.where(np.isnan(a), io | q, np.where(np.isnan(b), x | q, np.uint16(DNAN[dt]))).astype(np.uint16)
    return np.where(rnan, nan_out, out).astype(np.uint16)


def tree(op, dt, srcs, P, pairmask, nleaves, chain):
    """The engine's tree (msx_tree_dev.h tree_eval) over uint16 sources with
    combine() at every node: rounded at every node."""
    if chain:
        v = srcs[0].copy()
        for k in range(1, P):
            v = combine(op, dt, v, srcs[k])
        return v
    nl = nleaves or P
    v = [None] * P
    for k in range(nl):
        v[k] = srcs[2 * k].copy()
        if (pairmask >> k) & 1:
            v[k] = combine(op, dt, v[k], srcs[2 * k + 1])
    d = 1
    while d < P:
        for k in range(0, P - d, 2 * d):
            if k + d < nl:
                v[k] = combine(op, dt, v[k], v[k + d])
        d *= 2
    return v[0]


def partners(dt):
    """64 fixed partner bit patterns: +-0, +-inf, quiet and signalling NaNs
    with payload, min / max subnormal, min normal, max finite, +-1, 1 + ulp,
    and values whose sums with their neighbours tie."""
    if dt == "MSX_FLOAT16":
        mant, inf, one = 10, 0x7C00, 0x3C00
    else:
        mant, inf, one = 7, 0x7F80, 0x3F80
    q = 1 << (mant - 1)
    p = [0x0000, 0x8000, inf, 0x8000 | inf,
         inf | q | 1, 0x8000 | inf | q | 2, inf | 1, 0x8000 | inf | 3, inf | (q - 1), inf | q,   # qNaN / sNaN
         0x0001, 0x8001, (1 << mant) - 1, 0x8000 | ((1 << mant) - 1),                            # subnormals
         1 << mant, 0x8000 | (1 << mant), inf - 1, 0x8000 | (inf - 1),                           # min normal, max finite
         one, 0x8000 | one, one + 1, 0x8000 | (one + 1), one - 1, one + 2, one + 3]
    # ties: 1 + half an ulp of 2 (exponent one above, odd mantissa), and
    # small powers of two whose sum with values near 1 falls halfway
    e = 1 << mant
    for k in range(1, mant + 3):
        p.append(one - k * e)                 # 2^-k
        p.append(0x8000 | (one - k * e + 1))  # -(2^-k)(1+ulp)
    p += [one + e + 1, one + e + 3, one + 2 * e + 1, 0x8000 | (one + e + 1),
          inf - e, inf - e + 1, 0x8000 | (inf - e), (2 << mant) + 1, (3 << mant) + 1]
    # spread of exponents
    k = 0
    while len(p) < 64:
        p.append(((5 + 3 * k) << mant) % inf | (k * 37 % e) | (0x8000 if k & 1 else 0))
        k += 1
    p = p[:64]
    assert len(p) == 64
    return np.array(p, np.uint16)
