// msx_schedule.cpp — the pure schedule functions ("schedules" in
// msx_transport.h): algorithm gates, Rabenseifner blocks and the rank trees.
// Host arithmetic only; exported for the host-side tests.
#include "msx_transport.h"

#include <stdlib.h>
#include <string.h>

#include "msx_dtype.h"

namespace msx {

// ===========================================================================
// schedules
// ===========================================================================
int pof2_floor(int p)
{
    int v = 1;
    while (v * 2 <= p) v *= 2;
    return v;
}

int newrank_of(int rank, int p)
{
    const int rem = p - pof2_floor(p);
    if (rank < 2 * rem) return (rank & 1) ? rank / 2 : -1;
    return rank - rem;
}

int real_of_newrank(int n, int p)
{
    const int rem = p - pof2_floor(p);
    return n < rem ? 2 * n + 1 : n + rem;
}

int lineage_of(int me, int p)
{
    const int n = newrank_of(me, p);
    return n >= 0 ? n : newrank_of(me + 1, p);
}

Leaf leaf_of(int n, int p)
{
    // fold: odd rank 2n+1 computes MPID_Uop_call(tmp=x_{2n}, recvbuf=x_{2n+1})
    // (reduce.cpp:3858-3865): inout = x_{2n+1}, in = x_{2n}.
    const int rem = p - pof2_floor(p);
    Leaf l;
    if (n < rem) { l.a = 2 * n + 1; l.b = 2 * n; }
    else { l.a = n + rem; }
    return l;
}

// The flat communicators' algorithm switch points (Mpi.SwitchoverSettings
// [COLL_SWITCHOVER_FLAT], mpid/env.cpp:514-608): MPICH_DEFAULT_*_MSG override
// the coll.h defaults as env_to_int does (common/mpiutil.cpp:65-91): unset or
// longer than the 11-character buffer -> default, else _wtoi's value,
// clamped below at 0.  Read once; every rank must see the same environment,
// as with the reference.
namespace {
uint32_t env_switch(const char* name, int defval)
{
    const char* v = getenv(name);
    if (!v || strlen(v) > 11) return (uint32_t)defval;
    long long x = strtoll(v, nullptr, 10);           // _wtoi: leading blanks, sign, digits
    if (x > INT32_MAX) x = INT32_MAX;
    if (x < 0) x = 0;                                // minval 0
    return (uint32_t)x;
}
struct SwitchPoints {
    uint32_t allreduce_short = env_switch("MPICH_DEFAULT_ALLREDUCE_SHORT_MSG", 262144);
    uint32_t reduce_short = env_switch("MPICH_DEFAULT_REDUCE_SHORT_MSG", 65536);
    uint32_t redscat_long = env_switch("MPICH_DEFAULT_REDSCAT_COMMUTATIVE_LONG_MSG", 524288);
};
const SwitchPoints& switch_points()
{
    static const SwitchPoints sp;
    return sp;
}
}  // namespace

int allreduce_algo(int p, size_t count, int type_size, bool builtin)
{
    // reduce.cpp:3884-3888; count*type_size is evaluated in 32 bits.
    const uint32_t nbytes = (uint32_t)((uint64_t)count * (uint64_t)type_size);
    if (nbytes <= switch_points().allreduce_short || !builtin || count < (size_t)pof2_floor(p))
        return A_RECURSIVE_DOUBLING;
    return A_RABENSEIFNER;
}

int reduce_scatter_algo(int p, size_t total_count, int type_size, bool commutative)
{
    (void)p;
    if (!commutative) return -1;
    // reduce.cpp:1705-1709: nbytes = (unsigned)(total_count * type_size) wraps at 4 GiB.
    const uint32_t nbytes = (uint32_t)((uint64_t)total_count * (uint64_t)type_size);
    return nbytes < switch_points().redscat_long ? A_RS_HALVING : A_RS_PAIRWISE;
}

static int log2i(int v)
{
    int l = 0;
    while ((1 << l) < v) ++l;
    return l;
}

static int bitrev(int x, int bits)
{
    int r = 0;
    for (int i = 0; i < bits; ++i) r |= ((x >> i) & 1) << (bits - 1 - i);
    return r;
}

void allreduce_block(int p, size_t count, int j, size_t* start, size_t* len)
{
    const int pof2 = pof2_floor(p);
    const size_t rs = count / (size_t)pof2, es = count % (size_t)pof2;
    *start = (size_t)j * rs;
    *len = rs + (j == pof2 - 1 ? es : 0);   // endSize on the last block (:3935-3936)
}

// Recursive halving with mask = 1, 2, 4, ... keeps the lower half when the
// newrank bit is 0: the final block of newrank n is bitrev(n).
int allreduce_block_of_newrank(int p, int n) { return bitrev(n, log2i(pof2_floor(p))); }
int allreduce_block_owner(int p, int j) { return bitrev(j, log2i(pof2_floor(p))); }

static RankTree tree_from_leaves(int p, const int* leaf_newranks, int P)
{
    RankTree t;
    t.P = P;
    t.chain = false;
    t.pairmask = 0;
    for (int i = 0; i < 32; ++i) t.src[i] = -1;
    for (int k = 0; k < P; ++k) {
        Leaf l = leaf_of(leaf_newranks[k], p);
        t.src[2 * k] = l.a;
        if (l.b >= 0) {
            t.src[2 * k + 1] = l.b;
            t.pairmask |= 1u << k;
        }
    }
    return t;
}

RankTree tree_allreduce(int p, int n)
{
    const int P = pof2_floor(p);
    int lv[16];
    for (int k = 0; k < P; ++k) lv[k] = n ^ k;   // step mask pairs with n^mask
    return tree_from_leaves(p, lv, P);
}

RankTree tree_reduce_scatter(int p, int n)
{
    const int P = pof2_floor(p);
    const int bits = log2i(P);
    int lv[16];
    for (int k = 0; k < P; ++k) lv[k] = n ^ bitrev(k, bits);   // masks P/2, ..., 1
    return tree_from_leaves(p, lv, P);
}

int reduce_algo(int p, size_t count, int type_size, bool builtin)
{
    // reduce.cpp:151: (unsigned)(count*type_size) > reduce_short_msg (64 KiB by default)
    const uint32_t nbytes = (uint32_t)((uint64_t)count * (uint64_t)type_size);
    return (nbytes > switch_points().reduce_short && builtin && count >= (size_t)pof2_floor(p)) ? A_RABENSEIFNER
                                                                                                : A_BINOMIAL;
}

int gate_type_size(MPI_Datatype dt, bool nbc)
{
    if (dtype_is_derived(dt)) {            // user ops only; the builtin gates never see one
        const Dtype* t = dtype_lookup(dt);
        return t ? (int)(nbc ? t->extent : t->size) : 0;
    }
    return nbc ? type_size(dt) : (int)dtype_size(dt);
}

RankTree tree_reduce_rsag(int p, int n)
{
    // MPI_Reduce folds the ODD rank into the even one below it (reduce.cpp:
    // 136-165: Uop(tmp = x_{2n+1}, recvbuf = x_{2n})), newrank n -> real 2n.
    const int P = pof2_floor(p), rem = p - P;
    RankTree t;
    t.P = P;
    for (int i = 0; i < 32; ++i) t.src[i] = -1;
    for (int k = 0; k < P; ++k) {
        const int m = n ^ k;
        if (m < rem) {
            t.src[2 * k] = 2 * m;
            t.src[2 * k + 1] = 2 * m + 1;
            t.pairmask |= 1u << k;
        } else {
            t.src[2 * k] = m + rem;
        }
    }
    return t;
}

RankTree tree_ireduce_rsag(int p, int n, int root)
{
    // IreduceBuildScatterGatherTaskList (reduce.cpp:6267-6670) runs the same
    // fold and recursive halving over ranks RELATIVE TO THE ROOT: peer =
    // RankAdd(TrimmedToOriginalRankEven(rem, s ^ offset), root) (:6471), the
    // even relative rank combining Uop(tmp = x_{rel+1}, recvbuf) (:6403-6411).
    RankTree t = tree_reduce_rsag(p, n);
    for (int i = 0; i < 32; ++i)
        if (t.src[i] >= 0) t.src[i] = (t.src[i] + root) % p;
    return t;
}

RankTree tree_reduce_binomial(int p, int root)
{
    // relrank k receives from k|mask (reduce.cpp:489-537): a balanced tree over
    // relative ranks with the leaves >= p absent
    RankTree t;
    int P = 1;
    while (P < p) P *= 2;
    t.P = P;
    t.nleaves = p;
    for (int i = 0; i < 32; ++i) t.src[i] = -1;
    for (int k = 0; k < p; ++k) t.src[2 * k] = (k + root) % p;
    return t;
}

RankTree tree_pairwise(int p, int r)
{
    RankTree t;
    t.P = p;
    t.chain = true;
    for (int i = 0; i < 32; ++i) t.src[i] = -1;
    for (int k = 0; k < p; ++k) t.src[k] = ((r - k) % p + p) % p;   // src = r-1, r-2, ...
    return t;
}

// ---- the user-op collectives' combine plan (CombinePlan, msx_transport.h) ----
// One builder per reference schedule.  Each writes the value of ONE rank as the
// steps that compute it; a recursive builder returns the block that holds a
// partial value, having appended the steps that produce it.
namespace {
struct PlanBuilder {
    const int p;
    const bool commutative;
    CombinePlan plan;
    int step(int in, int io)
    {
        plan.steps.push_back({in, io});
        return io;
    }

    // Recursive doubling (reduce.cpp:3858-3925): the value of newrank n after
    // `level` steps.  Level 0 is the fold, the even rank below 2 * rem into the
    // odd rank above it.  At a step, a commutative op or a partner below
    // combines Uop(partner's, own); else "the sender is above us":
    // Uop(own, partner's) and the partner's copy takes the result.
    int doubled(int n, int level)
    {
        const int r = real_of_newrank(n, p);
        if (level == 0) return r < 2 * (p - pof2_floor(p)) ? step(r - 1, r) : r;
        const int mask = 1 << (level - 1);
        const int a = doubled(n, level - 1), b = doubled(n ^ mask, level - 1);
        return (commutative || real_of_newrank(n ^ mask, p) < r) ? step(b, a) : step(a, b);
    }
    // rank me's allreduce value; a folded even rank gets its odd neighbour's
    int allreduce(int me) { return doubled(lineage_of(me, p), log2i(pof2_floor(p))); }

    // The binomial tree at the root (reduce.cpp:440-540): relative ranks from
    // lroot = root (commutative) or 0; relrank rel receives from rel | mask and
    // combines Uop(child's, own) (commutative) or Uop(own, child's), the child's
    // copy taking the result.
    int reduce(int root)
    {
        const int lroot = commutative ? root : 0;
        std::vector<int> at((size_t)p);                      // the block holding relrank rel's value
        for (int rel = 0; rel < p; ++rel) at[(size_t)rel] = (rel + lroot) % p;
        for (int mask = 1; mask < p; mask <<= 1)
            for (int rel = 0; rel + mask < p; rel += 2 * mask) {
                int &own = at[(size_t)rel], &child = at[(size_t)(rel | mask)];
                own = commutative ? step(child, own) : step(own, child);
            }
        return at[0];
    }

    // Commutative reduce_scatter (reduce.cpp:917-1334), the partner's value
    // always `in`.  Pairwise: the blocks from ranks me - 1, me - 2, ... into
    // the rank's own.  Recursive halving with masks P / 2, ..., 1 after the
    // fold: a balanced tree over the leaves leaf_of(n ^ bitrev(k)) of the rank's
    // newrank n, as tree_reduce_scatter lists them for the kernels.
    int reduce_scatter(int me, int algo)
    {
        if (algo == A_RS_PAIRWISE) {
            for (int k = 1; k < p; ++k) step(((me - k) % p + p) % p, me);
            return me;
        }
        const int P = pof2_floor(p), bits = log2i(P), n = lineage_of(me, p);
        std::vector<int> v((size_t)P);
        for (int k = 0; k < P; ++k) {
            const Leaf l = leaf_of(n ^ bitrev(k, bits), p);
            v[(size_t)k] = l.b >= 0 ? step(l.b, l.a) : l.a;
        }
        for (int w = 1; w < P; w *= 2)
            for (int k = 0; k + w < P; k += 2 * w) step(v[(size_t)(k + w)], v[(size_t)k]);
        return v[0];
    }

    // Scan's recursive doubling (IscanBuildTaskList reduce.cpp:5285-5576): rank
    // r's partial after `level` steps.  At step mask it meets r ^ mask: the rank
    // above combines Uop(partner's, own), the rank below too when the op is
    // commutative, else Uop(own, partner's) and the partner's copy takes the
    // result.  The lower rank's last step feeds nothing and is not run.
    int partial(int r, int level)
    {
        if (level == 0) return r;
        const int mask = 1 << (level - 1), dst = r ^ mask;
        const bool last = (mask << 1) >= p;
        const int a = partial(r, level - 1);
        if (dst >= p || (last && r < dst)) return a;
        const int b = partial(dst, level - 1);
        return (r > dst || commutative) ? step(b, a) : step(a, b);
    }
    // rank me's result: its own contribution (scan) or nothing (exscan), then
    // Uop(partial of me ^ mask, result) at every step whose partner is below;
    // the first such step of an exscan takes the partial itself
    int scan(int me, bool exclusive)
    {
        int res = exclusive ? -1 : me, level = 0;
        for (int mask = 1; mask < p; mask <<= 1, ++level) {
            const int dst = me ^ mask;
            if (dst > me) continue;
            const int tmp = partial(dst, level);
            res = res < 0 ? tmp : step(tmp, res);
        }
        return res;
    }
};
}  // namespace

CombinePlan userop_plan(UserColl which, int p, int n, bool commutative, bool exclusive, size_t total_count,
                        int type_size)
{
    PlanBuilder b{p, commutative, {}};
    if (which == UserColl::reduce) b.plan.result = b.reduce(n);
    else if (which == UserColl::scan) b.plan.result = b.scan(n, exclusive);
    else if (which == UserColl::reduce_scatter && commutative)
        b.plan.result = b.reduce_scatter(n, reduce_scatter_algo(p, total_count, type_size, true));
    else b.plan.result = b.allreduce(n);      // non-commutative reduce_scatter: the allreduce of the whole vector
    return b.plan;
}

// The plans above written as one tree each, for an op with a tree function.
// in_left = 0: the engine's roles, left operand `inout`; in_left = 1: left
// operand `in`.
//   allreduce, commutative: doubled() makes the partner's value `in` and the
//     rank's own `inout` at every step, so rank n's value is tree_allreduce of
//     its newrank (a folded even rank takes its odd neighbour's); the fold is
//     (in = even rank, inout = odd rank), the odd rank in slot 2k.
//   allreduce, non-commutative: doubled() makes the lower newrank's value `in`
//     at every step, whichever rank asks: the tree over newranks 0..P-1 in
//     order with the left operand `in`, the fold pair (even, odd) in that order.
//   reduce: reduce()'s binomial tree over root-relative ranks (commutative,
//     in = right) or over ranks from 0 (non-commutative, in = left).
//   reduce_scatter, commutative: reduce_scatter()'s leaves are those of
//     tree_reduce_scatter, its chain tree_pairwise.
// tests/test_userop_plan_cpu.py evaluates both forms symbolically for every
// shape that has a tree and requires equal expressions.
bool devop_tree_spec(UserColl which, int p, int n, bool commutative, size_t total_count, int type_size, RankTree* t,
                     int* in_left)
{
    if (p < 2 || n < 0 || n >= p) return false;
    const bool as_allreduce = which == UserColl::allreduce || (which == UserColl::reduce_scatter && !commutative);
    if (as_allreduce) {
        if (p > 31) return false;
        if (commutative) {
            const int rem = p - pof2_floor(p);
            const int src = (n < 2 * rem && (n & 1) == 0) ? n + 1 : n;
            *t = tree_allreduce(p, newrank_of(src, p));
            *in_left = 0;
            return true;
        }
        const int P = pof2_floor(p), rem = p - P;
        RankTree r;
        r.P = P;
        for (int i = 0; i < 32; ++i) r.src[i] = -1;
        for (int k = 0; k < P; ++k) {
            const int odd = real_of_newrank(k, p);
            if (k < rem) {
                r.src[2 * k] = odd - 1;
                r.src[2 * k + 1] = odd;
                r.pairmask |= 1u << k;
            } else {
                r.src[2 * k] = odd;
            }
        }
        *t = r;
        *in_left = 1;
        return true;
    }
    if (which == UserColl::reduce) {
        if (p > 16) return false;
        *t = tree_reduce_binomial(p, commutative ? n : 0);
        *in_left = commutative ? 0 : 1;
        return true;
    }
    if (which != UserColl::reduce_scatter) return false;
    if (reduce_scatter_algo(p, total_count, type_size, true) == A_RS_PAIRWISE) {
        if (p > 16) return false;
        *t = tree_pairwise(p, n);
    } else {
        if (p > 31) return false;
        const int nr = newrank_of(n, p);
        *t = tree_reduce_scatter(p, nr >= 0 ? nr : newrank_of(n + 1, p));
    }
    *in_left = 0;
    return true;
}

}  // namespace msx
