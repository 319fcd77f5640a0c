"""The value a device tree function (MSX_Device_tree_function, include/msx.h)
must produce, in numpy -- written from the header's definition, not from the
library: leaf pairs, a balanced tree whose absent right subtrees pass the left
value up, or a left-deep chain, under either assignment of the operand roles.
Shared by the tests of msx_op_create_device_tree."""
import ctypes

import numpy as np


def nc(a, b, salt=0):
    """g(in = a, inout = b) = 3 * in - inout + salt, wrapping in the arrays' type"""
    t = a.dtype.type
    return (a * t(3) - b + t(salt)).astype(a.dtype)


def tree_value(s, P, pairmask, nleaves, chain, in_left, g=nc):
    """s[i] = the array in slot i (anything for a slot that is not to be read)."""
    def combine(left, right):
        return g(left, right) if in_left else g(right, left)

    if chain:
        v = s[0]
        for k in range(1, P):
            v = combine(v, s[k])
        return v
    present = nleaves if nleaves else P

    def subtree(first, width):
        if first >= present:
            return None
        if width == 1:
            return combine(s[2 * first], s[2 * first + 1]) if (pairmask >> first) & 1 else s[2 * first]
        left, right = subtree(first, width // 2), subtree(first + width // 2, width // 2)
        return left if right is None else combine(left, right)

    return subtree(0, P)


def devop_tree_spec(L, which, p, n, commutative, total_count, type_size):
    """msx_schedule_devop_tree -> (rc, src32, P, pairmask, nleaves, chain, in_left)"""
    src = (ctypes.c_int * 32)()
    P, nl, ch, il = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    pm = ctypes.c_uint()
    rc = L.msx_schedule_devop_tree(which, p, n, commutative, total_count, type_size, src, ctypes.byref(P),
                                   ctypes.byref(pm), ctypes.byref(nl), ctypes.byref(ch), ctypes.byref(il))
    return rc, list(src), P.value, pm.value, nl.value, ch.value, il.value


def spec_value(L, which, p, n, commutative, total_count, type_size, xs, g=nc):
    """The spec's value over xs[r] = rank r's contribution."""
    rc, src, P, pm, nl, ch, il = devop_tree_spec(L, which, p, n, commutative, total_count, type_size)
    assert rc == 0, (which, p, n, commutative)
    return tree_value([xs[r] if r >= 0 else None for r in src], P, pm, nl, ch, il, g)
