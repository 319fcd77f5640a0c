// msx_op_kind.h — which (builtin op, element kind) pairs have a kernel, and the
// C++ element type of each kind: stated once for every launcher (the streaming
// combine, the batched combine, the datatype accumulate, the fused tree).  The
// (op, kind) -> kernel mapping is stated here only.  A new kind still needs
// its Kind enumerator, kind_size() and kTypes row (msx_types), a new op its
// explicit tree_dispatch<OP> instantiation in a tree unit, and a new 16-bit
// kind msx_tree_half.hip / msx_tree_wide.hip.
//
// The launchers visit the map at compile time: for_op turns an op index into
// an OpTag, for_kind a Kind into a TypeTag, and the visitor (a generic lambda)
// instantiates its kernel launch on them (for_granule does the same for the
// byte movers' granule).  A pair outside the map never
// instantiates anything and gives hipErrorInvalidValue.  The rule restates the
// builtin ops' tables (op.cpp:739-1883) per kind; the handle-level legality
// (op_legal_groups, msx_types.cpp) is checked before any launcher is reached
// and is tied to this map by tests/test_op_kind_cpu.py.
//
// Included by .hip units only (msx_dev_ops.h is a device header).
#pragma once

#include "msx_dev_ops.h"

namespace msx {

template <int OP> struct OpTag { static constexpr int value = OP; };
template <class T> struct TypeTag { using type = T; };
template <int G> struct GranTag { static constexpr int value = G; };

// Classes of element kinds, as the ops' tables group them.
enum KindClass : unsigned {
    C_INT = 1,       // K_I8 .. K_U64
    C_FLOAT = 2,     // K_F32, K_F64
    C_HALF = 4,      // K_F16, K_BF16
    C_COMPLEX = 8,   // K_C32, K_C64
    C_BOOL = 16,     // K_BOOL, run as uint8_t
    C_LOC = 32,      // the six value/location structs
    C_ALL = 63
};

// The classes each op has an element-typed kernel for.
constexpr unsigned op_kind_classes(int op)
{
    switch (op) {
    case O_MAX: case O_MIN:               return C_INT | C_FLOAT | C_HALF;
    case O_SUM: case O_PROD:              return C_INT | C_FLOAT | C_HALF | C_COMPLEX;
    case O_LAND: case O_LOR: case O_LXOR: return C_INT | C_FLOAT | C_BOOL;
    case O_BAND: case O_BOR: case O_BXOR: return C_INT | C_BOOL;     // see op_bytewise
    case O_MAXLOC: case O_MINLOC:         return C_LOC;
    default:                              return 0;
    }
}

// BAND / BOR / BXOR are byte-independent: the combine, batch and tree paths run
// them on n * kind_size(k) raw bytes in 32-bit lanes, whatever the kind, and do
// not ask for_kind.  Only the datatype accumulate is element-typed for them.
constexpr bool op_bytewise(int op) { return op == O_BAND || op == O_BOR || op == O_BXOR; }

// MSX_SUM_WIDE on ONE combine is widen, one fp32 add, narrow: MPI_SUM's kernel
// on the 16-bit floats (msx.h), and no kernel for any other kind.
constexpr int single_combine_op(int opidx, Kind k)
{
    if (opidx != O_SUM_WIDE) return opidx;
    return (k == K_F16 || k == K_BF16) ? (int)O_SUM : (int)O_NULL;
}

// f(OpTag<OP>{}) for a builtin op that has kernels.
template <class F>
hipError_t for_op(int opidx, F&& f)
{
    switch (opidx) {
    case O_MAX:    return f(OpTag<O_MAX>{});
    case O_MIN:    return f(OpTag<O_MIN>{});
    case O_SUM:    return f(OpTag<O_SUM>{});
    case O_PROD:   return f(OpTag<O_PROD>{});
    case O_LAND:   return f(OpTag<O_LAND>{});
    case O_BAND:   return f(OpTag<O_BAND>{});
    case O_LOR:    return f(OpTag<O_LOR>{});
    case O_BOR:    return f(OpTag<O_BOR>{});
    case O_LXOR:   return f(OpTag<O_LXOR>{});
    case O_BXOR:   return f(OpTag<O_BXOR>{});
    case O_MINLOC: return f(OpTag<O_MINLOC>{});
    case O_MAXLOC: return f(OpTag<O_MAXLOC>{});
    default:       return hipErrorInvalidValue;
    }
}

// f(GranTag<G>{}) for the granule of a byte mover: a power of two <= 16 (the
// launchers check that before they ask).
template <class F>
hipError_t for_granule(int G, F&& f)
{
    switch (G) {
    case 16: return f(GranTag<16>{});
    case 8:  return f(GranTag<8>{});
    case 4:  return f(GranTag<4>{});
    case 2:  return f(GranTag<2>{});
    default: return f(GranTag<1>{});
    }
}

// f(TypeTag<T>{}) with the element type of `k`, if OP has a kernel for k's
// class and MASK keeps that class (the tree's per-op units mask out C_HALF,
// whose instantiations live in msx_tree_half.hip).
template <int OP, unsigned MASK = C_ALL, class F>
hipError_t for_kind(Kind k, F&& f)
{
    constexpr unsigned c = op_kind_classes(OP) & MASK;
    if constexpr ((c & C_INT) != 0) {
        switch (k) {
        case K_I8:  return f(TypeTag<int8_t>{});
        case K_U8:  return f(TypeTag<uint8_t>{});
        case K_I16: return f(TypeTag<int16_t>{});
        case K_U16: return f(TypeTag<uint16_t>{});
        case K_I32: return f(TypeTag<int32_t>{});
        case K_U32: return f(TypeTag<uint32_t>{});
        case K_I64: return f(TypeTag<int64_t>{});
        case K_U64: return f(TypeTag<uint64_t>{});
        default: break;
        }
    }
    if constexpr ((c & C_FLOAT) != 0) {
        if (k == K_F32) return f(TypeTag<float>{});
        if (k == K_F64) return f(TypeTag<double>{});
    }
    if constexpr ((c & C_HALF) != 0) {
        if (k == K_F16) return f(TypeTag<dev::f16>{});
        if (k == K_BF16) return f(TypeTag<dev::bf16>{});
    }
    if constexpr ((c & C_COMPLEX) != 0) {
        if (k == K_C32) return f(TypeTag<dev::c32>{});
        if (k == K_C64) return f(TypeTag<dev::c64>{});
    }
    if constexpr ((c & C_BOOL) != 0) {
        if (k == K_BOOL) return f(TypeTag<uint8_t>{});
    }
    if constexpr ((c & C_LOC) != 0) {
        switch (k) {
        case K_LOC_II: return f(TypeTag<dev::loc_ii>{});
        case K_LOC_FI: return f(TypeTag<dev::loc_fi>{});
        case K_LOC_SI: return f(TypeTag<dev::loc_si>{});
        case K_LOC_DI: return f(TypeTag<dev::loc_di>{});
        case K_LOC_FF: return f(TypeTag<dev::loc_ff>{});
        case K_LOC_DD: return f(TypeTag<dev::loc_dd>{});
        default: break;
        }
    }
    return hipErrorInvalidValue;
}

}  // namespace msx
