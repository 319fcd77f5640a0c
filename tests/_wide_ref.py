"""numpy definition of MSX_SUM_WIDE (msx.h): the fp32-accumulated tree sum of
MSX_FLOAT16 / MSX_BFLOAT16 sources.

This is the definition the kernels are held to, bit for bit; nothing here
comes from the library.  Sources and results are uint16 bit patterns.

  w(x), n(r)  as in _half_ref (exact widening to fp32, nearest-even narrowing);
              a NaN widens with its sign and payload as they are (mantissa
              bits moved to the top of the fp32 mantissa, nothing quieted);
  node        r = inout + in, one IEEE fp32 add on widened values (subnormals
              kept).  A NaN r follows the x86 rule in fp32, written out with
              integer operations: inout's bits | 0x00400000 if inout is a NaN,
              else in's bits | 0x00400000, else 0xFFC00000;
  tree        one tree of msx_reduce_tree_spec_dev's shape (leaf pairs, balanced
              tree with absent leaves, or chain), every node in fp32 and no
              rounding in between;
  root        n(root), or for a NaN root the truncation: sign, all-ones
              exponent, the top 10 (fp16) / 7 (bf16) mantissa bits.
"""
import numpy as np

from _half_ref import W, N, QBIT, DNAN, partners  # noqa: F401  (re-exported for the tests)

TYPES = ("MSX_FLOAT16", "MSX_BFLOAT16")
_MANT = {"MSX_FLOAT16": 10, "MSX_BFLOAT16": 7}
_INF = {"MSX_FLOAT16": 0x7C00, "MSX_BFLOAT16": 0x7F80}
QNAN32 = np.uint32(0x00400000)
DNAN32 = np.uint32(0xFFC00000)


def _isnan32(u):
    """fp32 bit patterns (uint32) -> NaN mask, by integer compare."""
    return (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)


def widen(dt, x):
    """uint16 patterns -> fp32 bit patterns (uint32): W[dt] for every non-NaN,
    sign | 0x7F800000 | payload << (23 - mantissa bits) for a NaN."""
    x = np.ascontiguousarray(x, dtype=np.uint16)
    m, inf = _MANT[dt], _INF[dt]
    nan = (x & np.uint16(0x7FFF)) > np.uint16(inf)
    safe = np.where(nan, np.uint16(0), x).astype(np.uint16)
    f = W[dt](safe).view(np.uint32)
    x32 = x.astype(np.uint32)
    nb = ((x32 & np.uint32(0x8000)) << np.uint32(16)) | np.uint32(0x7F800000) | \
        ((x32 & np.uint32((1 << m) - 1)) << np.uint32(23 - m))
    return np.where(nan, nb, f).astype(np.uint32)


def node(io, x):
    """fp32 SUM combine on bit patterns: new inout (uint32)."""
    a_nan, b_nan = _isnan32(io), _isnan32(x)
    a = np.where(a_nan, np.uint32(0), io).astype(np.uint32).view(np.float32)
    b = np.where(b_nan, np.uint32(0), x).astype(np.uint32).view(np.float32)
    with np.errstate(all="ignore"):
        r = (a + b).astype(np.float32).view(np.uint32)
    # inf + -inf: the only NaN two non-NaN operands make
    r = np.where(_isnan32(r), DNAN32, r)
    return np.where(a_nan, io | QNAN32, np.where(b_nan, x | QNAN32, r)).astype(np.uint32)


def root(dt, r):
    """fp32 bit patterns -> stored uint16 patterns."""
    m, inf = _MANT[dt], _INF[dt]
    nan = _isnan32(r)
    safe = np.where(nan, np.uint32(0), r).astype(np.uint32).view(np.float32)
    out = N[dt](safe)
    trunc = ((r >> np.uint32(16)) & np.uint32(0x8000)) | np.uint32(inf) | \
        ((r >> np.uint32(23 - m)) & np.uint32((1 << m) - 1))
    return np.where(nan, trunc.astype(np.uint16), out).astype(np.uint16)


def tree(dt, srcs, P, pairmask, nleaves, chain):
    """The engine's tree (msx_tree_dev.h tree_eval) over uint16 sources, every
    node in fp32, one narrowing at the root."""
    if chain:
        v = widen(dt, srcs[0])
        for k in range(1, P):
            v = node(v, widen(dt, srcs[k]))
        return root(dt, v)
    nl = nleaves or P
    v = [None] * P
    for k in range(nl):
        v[k] = widen(dt, srcs[2 * k])
        if (pairmask >> k) & 1:
            v[k] = node(v[k], widen(dt, srcs[2 * k + 1]))
    d = 1
    while d < P:
        for k in range(0, P - d, 2 * d):
            if k + d < nl:
                v[k] = node(v[k], v[k + d])
        d *= 2
    return root(dt, v[0])


def balanced(dt, srcs):
    """msx_reduce_tree_dev: the full balanced tree over p = 2^k sources."""
    p = len(srcs)
    slots = [None] * (2 * p)
    for k in range(p):
        slots[2 * k] = srcs[k]
    return tree(dt, slots, p, 0, 0, 0)
