// op_kind_test.cpp — ties csrc/msx_op_kind.h (which (op, kind) pairs have a
// kernel, and each kind's element type) to the host legality table of
// msx_types.cpp.  Host-only: compiled with hipcc --cuda-host-only, no GPU.
// Run by tests/test_op_kind_cpu.py, which parses the lines printed here.
#include <stdio.h>

#include "msx_op_kind.h"

using namespace msx;

static const char* const kKindNames[] = {
    "NONE", "I8", "U8", "I16", "U16", "I32", "U32", "I64", "U64", "F32", "F64", "BOOL", "C32", "C64",
    "LOC_II", "LOC_FI", "LOC_SI", "LOC_DI", "LOC_FF", "LOC_DD", "F16", "BF16", "COUNT"};
static_assert(sizeof(kKindNames) / sizeof(kKindNames[0]) == K_COUNT + 1, "one name per Kind");
static_assert(K_BOOL == 11 && K_LOC_II == 14 && K_F16 == 20, "names in the enum's order");

// The element type each kind must reach, stated here independently of the map
// (a kind mapped to another type of the same size would keep every sizeof).
template <class T>
static bool is_type_of(Kind k)
{
    using namespace dev;
    switch (k) {
    case K_I8:     return std::is_same<T, int8_t>::value;
    case K_U8:     return std::is_same<T, uint8_t>::value;
    case K_I16:    return std::is_same<T, int16_t>::value;
    case K_U16:    return std::is_same<T, uint16_t>::value;
    case K_I32:    return std::is_same<T, int32_t>::value;
    case K_U32:    return std::is_same<T, uint32_t>::value;
    case K_I64:    return std::is_same<T, int64_t>::value;
    case K_U64:    return std::is_same<T, uint64_t>::value;
    case K_F32:    return std::is_same<T, float>::value;
    case K_F64:    return std::is_same<T, double>::value;
    case K_BOOL:   return std::is_same<T, uint8_t>::value;
    case K_C32:    return std::is_same<T, c32>::value;
    case K_C64:    return std::is_same<T, c64>::value;
    case K_LOC_II: return std::is_same<T, loc_ii>::value;
    case K_LOC_FI: return std::is_same<T, loc_fi>::value;
    case K_LOC_SI: return std::is_same<T, loc_si>::value;
    case K_LOC_DI: return std::is_same<T, loc_di>::value;
    case K_LOC_FF: return std::is_same<T, loc_ff>::value;
    case K_LOC_DD: return std::is_same<T, loc_dd>::value;
    case K_F16:    return std::is_same<T, f16>::value;
    case K_BF16:   return std::is_same<T, bf16>::value;
    default:       return false;
    }
}

// sizeof the element type the map reaches for (opidx, k), or -1 for "no kernel";
// -2 (a failure) if the type is not the kind's.
template <unsigned MASK>
static int visit(int opidx, Kind k)
{
    int size = -1;
    bool right_type = true;
    const hipError_t e = for_op(opidx, [&](auto op) {
        return for_kind<decltype(op)::value, MASK>(k, [&](auto t) {
            using T = typename decltype(t)::type;
            size = (int)sizeof(T);
            right_type = is_type_of<T>(k);
            return hipSuccess;
        });
    });
    if (!right_type) {
        printf("FAIL visit(%d, %s): reached another type than the kind's\n", opidx, kKindNames[k]);
        return -2;
    }
    if (e == hipSuccess && size > 0) return size;
    if (e == hipErrorInvalidValue && size == -1) return -1;
    printf("FAIL visit(%d, %d): error %d, size %d\n", opidx, (int)k, (int)e, size);
    return -2;
}

int main()
{
    int fails = 0;

    // 1. every legal (op, predefined datatype) pair reaches a type of the table's size
    int ntypes = 0, legal = 0;
    const TypeInfo* types = type_table(&ntypes);
    for (int op = 0; op < O_COUNT; ++op) {
        for (int i = 0; i < ntypes; ++i) {
            const TypeInfo& t = types[i];
            if (op_check_dtype(op, t.handle) != MPI_SUCCESS) continue;
            ++legal;
            // MSX_SUM_WIDE reaches the map the way a single combine does
            const int size = visit<C_ALL>(single_combine_op(op, t.kind), t.kind);
            if (size != t.size || t.size != kind_size(t.kind)) {
                printf("FAIL %s %s: element of %d bytes, table %d, kind %d\n", op_name(op), t.name, size, t.size,
                       kind_size(t.kind));
                ++fails;
            }
        }
    }
    printf("TYPES %d\nLEGAL %d\n", ntypes, legal);

    // 2. the accepted (op, kind) set, one line per op index (K_NONE and K_COUNT included),
    //    and 3. what the tree's per-op units see of it
    for (int op = 0; op <= O_COUNT; ++op) {
        printf("OP %s", op == O_COUNT ? "O_COUNT" : op_name(op));
        for (int k = K_NONE; k <= K_COUNT; ++k) {
            const int size = visit<C_ALL>(op, (Kind)k);
            if (size == -2 || (size > 0 && size != kind_size((Kind)k))) ++fails;
            if (size > 0) printf(" %s", kKindNames[k]);
        }
        printf("\nTREE %s", op == O_COUNT ? "O_COUNT" : op_name(op));
        for (int k = K_NONE; k <= K_COUNT; ++k)
            if (visit<C_ALL & ~C_HALF>(op, (Kind)k) > 0) printf(" %s", kKindNames[k]);
        printf("\n");
    }

    // 4. MSX_SUM_WIDE on one combine
    for (int k = K_NONE; k <= K_COUNT; ++k) {
        const int want = (k == K_F16 || k == K_BF16) ? (int)O_SUM : (int)O_NULL;
        if (single_combine_op(O_SUM_WIDE, (Kind)k) != want || single_combine_op(O_MAX, (Kind)k) != O_MAX) {
            printf("FAIL single_combine_op kind %d\n", k);
            ++fails;
        }
    }
    printf("FAILS %d\n", fails);
    return fails ? 1 : 0;
}
