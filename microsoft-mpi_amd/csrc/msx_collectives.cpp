// msx_collectives.cpp — the collective schedules over the engine windows:
// the piece plan, the host user-op paths, one function per schedule of
// allreduce / reduce, reduce_scatter and scan / exscan, their
// dispatchers and the public engine_* entry points.
#include "msx_engine.h"

#include <algorithm>
#include <string.h>

namespace msx {

namespace {
// one OUT half of the two-step schedule: half the OUT area above the
// recursive-doubling results
size_t out_half_bytes(int p) { return ((chunk_bytes() - half_bytes(p)) / 2) & ~(size_t)255; }
// elements of esz bytes in `bytes`, whole 16-element granules
size_t granules(size_t bytes, size_t esz) { return (bytes / esz) & ~(size_t)15; }
int hip_rc(hipError_t e, const char* what) { return e == hipSuccess ? MPI_SUCCESS : hip_fail(e, what); }

RankTree rs_tree(int algo, int p, int me)
{
    return (algo == A_RS_PAIRWISE) ? tree_pairwise(p, me) : tree_reduce_scatter(p, lineage_of(me, p));
}
}  // namespace

// Elements per chunk of the pipelined two-step allreduce / reduce for p ranks
// and elements of esz bytes: p pieces of at most half an IN sub-slot each, the
// whole chunk within half the OUT area above the recursive-doubling results,
// whole 16-element pieces (0: the window is too small).
size_t two_step_chunk_el(int p, size_t esz)
{
    size_t pc_el = std::min((size_t)p * granules(half_bytes(p), esz), out_half_bytes(p) / esz);
    return pc_el - pc_el % ((size_t)p * 16);
}

// Rank me's part of the chunk [o, o + len) of a count-element vector: its
// piece [plo, phi) of the chunk (16-element granules) cut where the owner
// tree changes -- the owner of an element is
// that of its block in the WHOLE vector (allreduce_block, reduce.cpp:3927-
// 4066), so the chunking never changes a result.  Offsets are relative to
// the chunk start o.
void piece_plan(int p, size_t count, size_t o, size_t len, int me, Pieces* pc)
{
    const int pof2 = pof2_floor(p);
    pc->len = len;
    pc->pel = (((len + (size_t)p - 1) / (size_t)p) + 15) & ~(size_t)15;
    pc->plo = pc->lo(me);
    pc->phi = pc->hi(me);
    pc->ranges.clear();
    const size_t rs = count / (size_t)pof2;
    for (size_t e0 = pc->plo; e0 < pc->phi;) {
        const size_t ge = o + e0;                                             // global element
        const int j = rs ? (int)std::min((size_t)pof2 - 1, ge / rs) : pof2 - 1;
        size_t bst, bl;
        allreduce_block(p, count, j, &bst, &bl);
        const size_t e1 = std::min(pc->phi, bst + bl - o);
        pc->ranges.push_back({e0, e1, allreduce_block_owner(p, j)});
        e0 = e1;
    }
}

// ---- user-defined ops (host code): no GPU needed on these paths -------------
namespace {

// reduce_scatter's blocks: block r is recvcounts[r] elements, disp[r] elements
// into the input; hold: where an in-place call keeps its results
struct RsBlocks {
    const int* recvcounts = nullptr;
    std::vector<size_t> disp;
    size_t maxcnt = 0, mycnt = 0, total = 0;
    bool in_place = false;
    char* hold = nullptr;
    size_t cnt(int r) const { return (size_t)recvcounts[r]; }
};

// The host user-op entry points: each names its plan (userop_plan,
// msx_schedule.cpp) and the elements it combines and stores; host_user_run
// (msx_engine.cpp) gathers and executes.
//
// MPI_Reduce_scatter.  Commutative: the builtin schedules (recursive halving or
// pairwise, same 32-bit gate, reduce.cpp:917-1334) over the rank's own block
// of every contribution.  Non-commutative: recursive doubling over the whole
// vector (MPIR_Reduce_scatter_non_commutative, reduce.cpp:1340-1630) -- for a
// power-of-two p each block is exactly the recursive-doubling allreduce value;
// other p share its lower-first order -- then block `me` of the result.
int host_user_reduce_scatter(Comm* c, const char* src, void* recvbuf, const RsBlocks& b, MPI_Datatype dt,
                             const OpRef& op)
{
    const int me = c->rank;
    const CombinePlan plan = userop_plan(UserColl::reduce_scatter, c->size, me, op.commutative, false, b.total,
                                         gate_type_size(dt, false));
    const size_t first = op.commutative ? b.disp[me] : 0, count = op.commutative ? b.mycnt : b.total;
    return host_user_run(c, src, recvbuf, b.total, dt, op, b.mycnt ? &plan : nullptr, first, count, b.disp[me],
                         b.mycnt);
}

}  // namespace

// MPI_Reduce with a user function (host code): the reference's binomial tree
// (reduce.cpp:440-540) at the root; every other rank only contributes.
int host_user_reduce(Comm* c, const void* sendbuf, void* recvbuf, size_t count, MPI_Datatype dt,
                     const OpRef& op, int root)
{
    const CombinePlan plan = userop_plan(UserColl::reduce, c->size, root, op.commutative, false, count, 0);
    return host_user_run(c, sendbuf == MPI_IN_PLACE ? recvbuf : sendbuf, recvbuf, count, dt, op,
                         c->rank == root ? &plan : nullptr, 0, count, 0, count);
}

namespace {

// MPI_Scan / MPI_Exscan: the recursive-doubling task list of the reference
// (IscanBuildTaskList reduce.cpp:5285-5576, IexscanBuildTaskList :5671-5960,
// NbcTask::ExecuteScan tasks.cpp:694-766), every combine with the reference's
// operands and roles.  Rank 0 of an exscan has no value: recvbuf undefined.
int host_user_scan(Comm* c, const void* sendbuf, void* recvbuf, size_t count, MPI_Datatype dt,
                   const OpRef& op, bool exclusive)
{
    const CombinePlan plan = userop_plan(UserColl::scan, c->size, c->rank, op.commutative, exclusive, count, 0);
    return host_user_run(c, sendbuf == MPI_IN_PLACE ? recvbuf : sendbuf, recvbuf, count, dt, op, &plan, 0, count, 0,
                         count);
}

// ---- what the window schedules share ---------------------------------------

size_t up256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }   // whole 256-byte lines

// Everything one window call shares, and the schedules as its members: the
// transport and this rank's place in it, the op and element type, the stream,
// the windows and the operands.  A schedule reads these and its own
// arguments, nothing else.
struct Call {
    Transport* tp;
    int p, me, opidx;
    Kind k;
    size_t esz;
    hipStream_t s;
    const char* src;             // the input (recvbuf when in place)
    char* dst;                   // recvbuf
    int root = -1;               // >= 0: only `root` receives the result (MPI_Reduce)
    bool want = true, nbc = false;   // this rank receives the result; a non-blocking call
    Windows w;
    BufInfo bs, bd;              // host buffers: device aliases for the call
    char* stage = nullptr;       // device scratch for operands the kernels cannot address

    // host buffers: device aliases for the call (pinned in place of staging);
    // `pins` lives in the dispatcher, past the schedule: its destructor syncs
    // the streams before the pins are released
    void alias_operands(PinHold& pins, size_t src_bytes, void* out, size_t out_bytes, hipStream_t aux = nullptr)
    {
        bs = classify(src);
        bd = classify(dst);
        pins.sync_before_release(s);
        if (aux) pins.sync_before_release(aux);
        alias_host_operands(pins, true, src, src_bytes, &bs, out, out_bytes, &bd);
    }
    const char* srcv() const { return bs.place == Place::Device ? static_cast<const char*>(bs.dev) : src; }
    char* dstv() const { return bd.place == Place::Device ? static_cast<char*>(bd.dev) : dst; }
    // a peer that receives my contribution whole / my results
    bool receives(int r) const { return r != me && (root < 0 || r == root); }
    // every rank's contribution as this rank reads it: the sub-slots of my IN
    // area, `half` bytes in
    std::vector<char*> in_subs(size_t half = 0) const
    {
        std::vector<char*> subs((size_t)p);
        for (int r = 0; r < p; ++r) subs[r] = w.sub(me, r) + half;
        return subs;
    }
    // the ranks my results go to, this rank first when it receives
    std::vector<int> result_dests() const
    {
        std::vector<int> dests;
        if (want) dests.push_back(me);
        for (int r = 0; r < p; ++r)
            if (receives(r)) dests.push_back(r);
        return dests;
    }
    // My piece of a chunk, one launch per owner tree, from `subs` into the OUT
    // area of every receiver, `obase` bytes in; tw: what the last launch posts.
    int run_pieces(const Pieces& pc, const std::vector<char*>& subs, const std::vector<int>& dests, size_t obase,
                   const TreeWait* tw = nullptr) const
    {
        int rc = MPI_SUCCESS;
        for (size_t i = 0; i < pc.ranges.size() && rc == MPI_SUCCESS; ++i) {
            const TwoStepRange& g = pc.ranges[i];
            std::vector<char*> extra;
            for (size_t d = 1; d < dests.size(); ++d) extra.push_back(w.out(dests[d]) + obase + g.e0 * esz);
            // the owner's Rabenseifner tree: allreduce, MPI_Reduce or MPI_Ireduce
            const RankTree t = root < 0 ? tree_allreduce(p, g.owner)
                                        : (nbc ? tree_ireduce_rsag(p, g.owner, root) : tree_reduce_rsag(p, g.owner));
            rc = run_rank_tree(opidx, k, t, subs, esz, g.e0 - pc.plo, g.e1 - g.e0,
                               w.out(dests[0]) + obase + g.e0 * esz, s, extra, tw);
        }
        return rc;
    }

    int allreduce_flag_small(const RankTree& t, size_t count) const;
    int allreduce_rd_barrier(const RankTree& t, size_t count, size_t qmax) const;
    int allreduce_two_step(size_t count, size_t pc_el) const;
    int allreduce_rsag_barrier(size_t count, size_t qmax) const;
    int reduce_scatter_flags(const RankTree& t, const RsBlocks& b, size_t qh_el) const;
    int reduce_scatter_barrier(const RankTree& t, const RsBlocks& b, size_t qe) const;
    int scan_flags(size_t count, bool exclusive) const;
    int scan_barrier(size_t count, bool exclusive, size_t ce) const;
};

// The scope of one GPU-flag call: the pinned error word its flag waits report
// through, the push counter, the sequence numbers, the "half free" guard of
// the pipelined schedules and the call's one host sync.  Toggling rd_parity
// and out_quiet stay with the schedule that owns them.
struct FlagCall {
    const Call& c;
    const char* op;                  // leads the error texts
    int *err_host = nullptr, *err_dev = nullptr;
    unsigned* counter = nullptr;
    std::vector<unsigned long long*> done_to;            // my GPU done flag in every peer's window

    int no_mem() const { set_error("%s: flag word allocation failed", op); return MPI_ERR_NO_MEM; }
    int need_counter() { return (counter = c.tp->push_counter()) ? MPI_SUCCESS : no_mem(); }
    int begin(bool with_counter = true)
    {
        if (!(err_dev = wait_err_word(&err_host))) return no_mem();
        *err_host = 0;
        return with_counter ? need_counter() : MPI_SUCCESS;
    }
    unsigned long long seq() { return ++c.tp->rd_seq; }
    // The IN / OUT halves that chunk or round i (sequence number seq) writes
    // are free once every peer finished seq - 2.  The first two of a call are
    // guarded on the host by the previous flag calls' post_done; later ones
    // wait on the GPU, one workgroup, for the peers' "done" flags.
    int half_free(size_t i, unsigned long long seq, int rc)
    {
        if (i < 2) {
            for (int r = 0; r < c.p && rc == MPI_SUCCESS; ++r)
                if (r != c.me && seq > 2) rc = c.tp->wait_done(r, seq - 2);
        } else if (rc == MPI_SUCCESS) {
            rc = hip_rc(launch_push_wait(nullptr, nullptr, nullptr, 0, nullptr, 0, seq - 2, nullptr,
                                         c.w.flags(c.me) + kDoneFlags, c.p, c.me, err_dev, c.s, 3),
                        (std::string(op) + " half-free wait").c_str());
        }
        return rc;
    }
    // my "done" flag of seq into every peer's window, after my reads of its
    // halves in stream order
    int post_half_done(unsigned long long seq)
    {
        if (done_to.empty())
            for (int r = 0; r < c.p; ++r)
                if (r != c.me) done_to.push_back(c.w.flags(r) + kDoneFlags + c.me);
        return hip_rc(launch_post_flags(done_to.data(), (int)done_to.size(), seq, c.s),
                      (std::string(op) + " done flags").c_str());
    }
    // The flag schedules' synchronisation point, one k_push_wait launch: the
    // ranges of sg into the peers' windows, then seq into the flags fl; one
    // workgroup waits until wait_n peers' arrival flags in my window reached seq.
    int push(const Segs& sg, const std::vector<unsigned long long*>& fl, unsigned long long seq, int wait_n,
             const char* what)
    {
        return hip_rc(launch_push_wait(sg.src.data(), sg.dst.data(), sg.n.data(), (int)sg.src.size(), fl.data(),
                                       (int)fl.size(), seq, counter ? counter + kCountWords : nullptr,
                                       c.w.flags(c.me), wait_n, c.me, err_dev, c.s), what);
    }
    // the call's host sync, a flag wait's timeout report, then this rank's
    // completion word: nothing of it reads the halves of `seq` any more
    int finish(int rc, unsigned long long seq, const char* sync_what, const char* op_name, bool index_is_rank = true)
    {
        const int rs = sync_stream(c.s, sync_what);
        if (rc == MPI_SUCCESS) rc = rs;
        if (rc == MPI_SUCCESS && __atomic_load_n(err_host, __ATOMIC_ACQUIRE))
            rc = flag_timeout(op_name, c.me, __atomic_load_n(err_host, __ATOMIC_ACQUIRE), seq, index_is_rank);
        c.tp->post_done(seq);
        c.tp->window_open = true;
        return rc;
    }
};

// ---- allreduce / reduce -----------------------------------------------------

// Flag small call: a recursive-doubling (or binomial) call that fits half a
// sub-slot; t is the tree this rank evaluates.
int Call::allreduce_flag_small(const RankTree& t, size_t count) const
{
    // No host barrier at all.  Each rank pushes its vector into the IN
    // half of every rank that evaluates a tree (all peers for
    // allreduce, the root for reduce) and posts the call's sequence
    // number into their flag slots; ONE workgroup of the same launch
    // (k_push_wait) waits on the GPU until all peers' flags reached the
    // sequence, and the tree follows in stream order.  (Rounds 1-2 let
    // every tree workgroup spin on the flags instead, one launch less;
    // with a multi-MiB tree spinning, five ranks sharing one GPU starved
    // each other's pushes until the 20 s bound.)
    // A half is reused two calls later: before pushing call s into
    // rank r's half, this rank waits (host, shared memory) until r has
    // posted that it finished call s-2 -- normally long since true.
    const size_t half = (size_t)tp->rd_parity * half_bytes(p);
    std::vector<char*> subs = in_subs(half);
    // small host buffers go through the engine's pinned bounce buffers
    // (CPU copies in and out, the kernels read / write them over PCIe)
    // instead of synchronous pageable copies through HBM staging
    const size_t nbytes = count * esz;
    const bool bounce_src = bs.place != Place::Device && nbytes <= bounce_max_bytes() &&
                            engine_bounce(0).get(nbytes);
    const bool bounce_dst = want && bd.place != Place::Device && nbytes <= bounce_max_bytes() &&
                            engine_bounce(1).get(nbytes);
    const char* mine = nullptr;
    int rc = MPI_SUCCESS;
    if (bounce_src) {
        memcpy(engine_bounce(0).host, src, nbytes);
        mine = engine_bounce(0).dev;
    } else {
        rc = device_view(bs, src, 0, nbytes, stage, s, &mine);
    }
    FlagCall fc{*this, "allreduce"};
    const unsigned long long seq = fc.seq();
    Segs sg;
    std::vector<unsigned long long*> fl;
    for (int r = 0; r < p && rc == MPI_SUCCESS; ++r)
        if (receives(r)) {
            if (seq > 2) rc = tp->wait_done(r, seq - 2);
            sg.add(mine, w.sub(r, me) + half, count * esz);
            if (!fault_drop_flags(me, seq)) fl.push_back(w.flags(r) + me);
        }
    subs[(size_t)me] = const_cast<char*>(mine);
    int ra = fc.begin(false);
    if (ra != MPI_SUCCESS) return ra;
    char* out = bd.place == Place::Device ? static_cast<char*>(bd.dev)
                                          : (bounce_dst ? engine_bounce(1).dev : w.out(me));
    // a rank that pushes nothing asks for no push counter
    if (rc == MPI_SUCCESS && !sg.src.empty() && (ra = fc.need_counter()) != MPI_SUCCESS) return ra;
    if (rc == MPI_SUCCESS) rc = fc.push(sg, fl, seq, want ? p : 0, "allreduce push");
    if (rc == MPI_SUCCESS && want) {
        rc = run_rank_tree(opidx, k, t, subs, esz, 0, count, out, s);   // after the wait, in stream order
        if (rc == MPI_SUCCESS && out == w.out(me)) rc = copy_async(dst, out, count * esz, s);
    }
    // post_done: this rank's tree no longer reads the half
    rc = fc.finish(rc, seq, "allreduce tree", root < 0 ? "allreduce" : "reduce");
    if (rc == MPI_SUCCESS && bounce_dst) memcpy(dst, engine_bounce(1).host, nbytes);
    tp->rd_parity ^= 1;
    trace("allreduce: done (GPU arrival flags, seq %llu) rc=%d", seq, rc);
    return rc;
}

// Host-barrier recursive doubling / binomial: chunks of one sub-slot, each
// rank that evaluates a tree gets every contribution whole.
int Call::allreduce_rd_barrier(const RankTree& t, size_t count, size_t qmax) const
{
    std::vector<char*> subs = in_subs();
    int rc = MPI_SUCCESS;
    for (size_t o = 0; o < count && rc == MPI_SUCCESS; o += qmax) {
        const size_t len = std::min(qmax, count - o);
        const char* mine = nullptr;
        rc = device_view(bs, src, o * esz, len * esz, stage, s, &mine);
        Segs sg;                      // my own contribution is read in place
        for (int r = 0; r < p; ++r)
            if (receives(r)) sg.add(mine, w.sub(r, me), len * esz);
        subs[(size_t)me] = const_cast<char*>(mine);
        if (rc == MPI_SUCCESS) rc = sg.run(s, "allreduce push");
        if (rc == MPI_SUCCESS) rc = sync_stream(s, "allreduce push");
        if (rc == MPI_SUCCESS) rc = tp->barrier();                              // A
        if (rc == MPI_SUCCESS && want) {
            char* out = bd.place == Place::Device ? static_cast<char*>(bd.dev) + o * esz : w.out(me);
            rc = run_rank_tree(opidx, k, t, subs, esz, 0, len, out, s);
            if (rc == MPI_SUCCESS && out == w.out(me)) rc = copy_async(dst + o * esz, out, len * esz, s);
            if (rc == MPI_SUCCESS) rc = sync_stream(s, "allreduce tree");
        }
        if (rc == MPI_SUCCESS) rc = tp->barrier();                              // B
    }
    trace("allreduce: done rc=%d", rc);
    return rc;
}

// Two-step (GPU flags): Rabenseifner in two GPU-synchronised steps per chunk
// of pc_el elements.
int Call::allreduce_two_step(size_t count, size_t pc_el) const
{
    // Barrier-free Rabenseifner: the same pieces, trees and result
    // placement as the host-barrier schedule below, synchronised on the
    // GPU, chunk by chunk with no host synchronisation between chunks.
    // Per chunk (elements [o, o + len), pieces cut in 16-element granules):
    //  0. (chunks >= 2) one workgroup waits until every peer posted that it
    //     finished chunk seq - 2 (its GPU "done" flag): the IN / OUT halves
    //     this chunk writes are free.  The first two chunks of a call are
    //     guarded on the host by the previous flag calls' post_done.
    //  1. k_push_wait: piece r of my chunk -> rank r's IN half, then its
    //     arrival flag; one workgroup waits for every peer's piece of mine.
    //  2. my piece evaluated (one launch per owner tree, owners by GLOBAL
    //     element, reduce.cpp:3941-4065) into the OUT half of every
    //     receiver; the last workgroup posts result-ready flags (tree_done).
    //  3. receivers: one workgroup waits for every peer's result flag,
    //     then the OUT half is copied into recvbuf + o.
    //  4. (when a later chunk of this call reuses the halves) my "done"
    //     flag into every peer's window, after the copy in stream order.
    // Halves alternate with rd_parity per chunk.  One host sync per call
    // (rounds 1-3 paid five per 512 MiB chunk on the host-barrier path).
    // Only single workgroups spin, so ranks sharing a GPU cannot starve
    // each other's pushes.
    int rc = MPI_SUCCESS;
    if (!tp->out_quiet && (rc = tp->barrier()) != MPI_SUCCESS) return rc;
    FlagCall fc{*this, "allreduce"};
    if ((rc = fc.begin()) != MPI_SUCCESS) return rc;
    const size_t Qh = half_bytes(p), out_half = out_half_bytes(p);
    const std::vector<int> dests = result_dests();
    const size_t nchunks = (count + pc_el - 1) / pc_el;
    unsigned long long seq = 0;
    size_t nranges = 0;
    Pieces pc;
    for (size_t ci = 0; ci < nchunks && rc == MPI_SUCCESS; ++ci) {
        const size_t o = ci * pc_el;
        piece_plan(p, count, o, std::min(pc_el, count - o), me, &pc);
        const size_t half = (size_t)tp->rd_parity * Qh;
        const size_t obase = Qh + (size_t)tp->rd_parity * out_half;
        const char* mine = nullptr;
        rc = device_view(bs, src, o * esz, pc.len * esz, stage, s, &mine);
        seq = fc.seq();
        rc = fc.half_free(ci, seq, rc);
        if (rc != MPI_SUCCESS) break;
        Segs sg;
        std::vector<unsigned long long*> fl, done;
        for (int r = 0; r < p; ++r) {
            if (r == me || pc.hi(r) <= pc.lo(r)) continue;
            sg.add(mine + pc.lo(r) * esz, w.sub(r, me) + half, (pc.hi(r) - pc.lo(r)) * esz);
            if (!fault_drop_flags(me, seq)) fl.push_back(w.flags(r) + me);
        }
        for (int d : dests)
            if (d != me) done.push_back(w.flags(d) + kResultFlags + me);
        nranges += pc.ranges.size();
        std::vector<char*> subs = in_subs(half);
        subs[(size_t)me] = const_cast<char*>(mine) + pc.plo * esz;
        // step 1: push my pieces and their arrival flags; one workgroup
        // waits for the peers' pieces of mine (none when my piece is empty)
        rc = fc.push(sg, fl, seq, pc.ranges.empty() ? 0 : p, "allreduce push");
        // step 2: my piece into every receiver's OUT half; the last
        // workgroup of the last launch posts the result flags
        if (rc == MPI_SUCCESS && pc.ranges.empty() && !done.empty())
            rc = hip_rc(launch_post_flags(done.data(), (int)done.size(), seq, s), "allreduce result flags");
        const TreeWait tw{fc.counter + 2 * kCountWords, (unsigned)pc.ranges.size(), &done, seq};
        if (rc == MPI_SUCCESS) rc = run_pieces(pc, subs, dests, obase, &tw);
        if (rc == MPI_SUCCESS && want) {
            // step 3: every peer's result in my OUT half, then into recvbuf
            rc = hip_rc(launch_push_wait(nullptr, nullptr, nullptr, 0, nullptr, 0, seq, nullptr,
                                         w.flags(me) + kResultFlags, p, me, fc.err_dev, s, 2), "allreduce result wait");
            if (rc == MPI_SUCCESS) rc = copy_async(dstv() + o * esz, w.out(me) + obase, pc.len * esz, s);
        }
        // step 4: this chunk's halves are free again (read by my trees and
        // my copy, both earlier on the stream) -- only a later chunk of
        // this call waits on it
        if (rc == MPI_SUCCESS && ci + 2 < nchunks) rc = fc.post_half_done(seq);
        tp->rd_parity ^= 1;
    }
    ++g_stats.flag_calls;
    rc = fc.finish(rc, seq, "allreduce two-step", root < 0 ? "allreduce" : "reduce");
    tp->out_quiet = true;
    trace("allreduce: done (two-step, GPU flags, %zu chunk(s), last seq %llu, %zu ranges) rc=%d", nchunks, seq,
          nranges, rc);
    return rc;
}

// Host-barrier Rabenseifner, chunks of p sub-slots.
int Call::allreduce_rsag_barrier(size_t count, size_t qmax) const
{
    // Rabenseifner order: element e belongs to block j(e), whose value the
    // reference computes at newrank bitrev(j).  Each chunk is cut into p
    // pieces (work balance only, 16-element granules); each element of a piece
    // is evaluated with the tree of its block's owner.
    const size_t ce = (size_t)p * qmax;
    hipStream_t s2 = aux_stream(tp) ? aux_stream(tp) : s;
    std::vector<char*> subs = in_subs();
    Pieces pc;
    int rc = MPI_SUCCESS;
    for (size_t o = 0; o < count && rc == MPI_SUCCESS; o += ce) {
        const double t0 = now_s();
        piece_plan(p, count, o, std::min(ce, count - o), me, &pc);
        const char* mine = nullptr;
        rc = device_view(bs, src, o * esz, pc.len * esz, stage, s, &mine);
        Segs scatter;
        for (int r = 0; r < p; ++r)                  // my own piece is read in place
            if (r != me) scatter.add(mine + pc.lo(r) * esz, w.sub(r, me), (pc.hi(r) - pc.lo(r)) * esz);
        subs[(size_t)me] = const_cast<char*>(mine) + pc.plo * esz;
        if (rc == MPI_SUCCESS) rc = scatter.run(s, "allreduce scatter");
        if (rc == MPI_SUCCESS) rc = sync_stream(s, "allreduce scatter");
        const double t1 = now_s();
        if (rc == MPI_SUCCESS) rc = sync_stream(s2, "allreduce collect");           // OUT(me) free
        if (rc == MPI_SUCCESS) rc = tp->barrier();                                  // A
        const double t2 = now_s();
        if (rc != MPI_SUCCESS) break;
        // reduce my piece from my IN area (local) and store the result straight
        // into every receiver's OUT area: the push is fused into the tree
        // kernel (remote stores over xGMI)
        rc = run_pieces(pc, subs, result_dests(), 0);
        if (rc == MPI_SUCCESS) rc = sync_stream(s, "allreduce push");
        const double t3 = now_s();
        if (rc == MPI_SUCCESS) rc = tp->barrier();                                  // B
        const double t4 = now_s();
        g_stats.chunks += 1;
        g_stats.t[0] += t1 - t0;
        g_stats.t[1] += t2 - t1;
        g_stats.t[2] += t3 - t2;
        g_stats.t[3] += t4 - t3;
        // collect on a second stream: it overlaps the next chunk's scatter
        // (local HBM copy vs xGMI writes); synced before the next barrier A
        if (rc == MPI_SUCCESS && want) rc = copy_async(dst + o * esz, w.out(me), pc.len * esz, s2);
    }
    const double tc = now_s();
    if (rc == MPI_SUCCESS) rc = sync_stream(s2, "allreduce collect");
    g_stats.t[4] += now_s() - tc;
    g_stats.calls += 1;
    trace("allreduce: done rc=%d", rc);
    return rc;
}

}  // namespace

// The dispatcher.  root < 0: allreduce; root >= 0: only `root` receives the
// result (MPI_Reduce).
int do_allreduce(Comm* comm, const void* sendbuf, void* recvbuf, size_t count, MPI_Datatype dt,
                 const OpRef& op, int root, bool nbc)
{
    // device user ops stay in HBM (msx_devop.cpp); MPI_Op_create's functions
    // are host code: no GPU needed on that path
    if (op.dev_fn) return devop_allreduce(comm, sendbuf, recvbuf, count, dt, op);
    if (op.opidx == O_NULL) return host_user_allreduce(comm, sendbuf, recvbuf, count, dt, op);
    int rc = ensure_device();
    if (rc != MPI_SUCCESS) return rc;

    Transport* tp = comm->tp;
    if (rccl_requested())
        if (ncclComm_t rcomm = rccl_comm(tp)) return rccl_allreduce(rcomm, comm, sendbuf, recvbuf, count, dt, op, root, nbc);
    const int p = comm->size, me = comm->rank;
    const size_t esz = (size_t)type_info(dt)->size;
    Call c{tp, p, me, op.opidx, type_info(dt)->kind, esz, tp->stream(),
           static_cast<const char*>(sendbuf == MPI_IN_PLACE ? recvbuf : sendbuf), static_cast<char*>(recvbuf),
           root, root < 0 || root == me, nbc};
    const int gate = gate_type_size(dt, nbc);
    const int algo = root >= 0 ? reduce_algo(p, count, gate, true) : allreduce_algo(p, count, gate, true);
    const bool rd = algo == A_RECURSIVE_DOUBLING || algo == A_BINOMIAL;
    // A recursive-doubling (or binomial) call that fits half a sub-slot runs
    // barrier-free at its end: it uses the IN half `rd_parity`, alternating per
    // call.  Pushing into a peer's half P again (two calls later) happens only
    // after this rank passed the previous call's barrier A, which that peer
    // reached only after finishing its tree on half P.
    const bool rd_single = rd && count * esz <= (half_bytes(p) & ~(size_t)(16 * esz - 1)) && p <= 32 && tp->has_done();
    // Rabenseifner in two GPU-synchronised steps per chunk (allreduce_two_step): a
    // chunk is p pieces of at most half an IN sub-slot each and fits half the
    // OUT area above the recursive-doubling results; a longer message runs as
    // a pipeline of such chunks.  Only count, type, p and the environment
    // decide, so every rank takes the same branch and the same chunks.
    const size_t pc_el = two_step_chunk_el(p, esz);
    const bool two_step = algo == A_RABENSEIFNER && p >= 2 && p <= 32 && tp->has_done() &&
                          count * esz <= two_step_max(tp) && pc_el > 0;
    if ((rc = get_windows(tp, &c.w, rd_single || two_step)) != MPI_SUCCESS) return rc;
    PinHold pins;
    c.alias_operands(pins, count * esz, c.want ? c.dst : nullptr, c.want ? count * esz : 0, aux_stream(tp));
    // elements per sub-slot, whole 16-element granules
    const size_t qmax = granules(c.w.Q, esz);
    if (qmax == 0) { set_error("allreduce: window too small"); return MPI_ERR_INTERN; }
    if (c.bs.place != Place::Device) {
        c.stage = dev_scratch(std::min(count, (size_t)p * qmax) * esz);
        if (!c.stage) { set_error("allreduce: scratch allocation failed"); return MPI_ERR_NO_MEM; }
    }
    trace("allreduce: count=%zu esz=%zu algo=%d qmax=%zu", count, esz, algo, qmax);
    if (rd) {
        // every rank that evaluates a tree needs every contribution whole:
        // recursive doubling -> all ranks evaluate their own lineage's tree;
        // binomial reduce -> only the root evaluates
        const RankTree t = (algo == A_BINOMIAL) ? tree_reduce_binomial(p, root) : tree_allreduce(p, lineage_of(me, p));
        return rd_single ? c.allreduce_flag_small(t, count) : c.allreduce_rd_barrier(t, count, qmax);
    }
    return two_step ? c.allreduce_two_step(count, pc_el) : c.allreduce_rsag_barrier(count, qmax);
}

namespace {

// ---- reduce_scatter ---------------------------------------------------------

// One-step (GPU flags): rounds of qh_el elements per block; `stage` holds a
// host-resident input whole.
int Call::reduce_scatter_flags(const RankTree& t, const RsBlocks& b, size_t qh_el) const
{
    FlagCall fc{*this, "reduce_scatter"};
    int rc = fc.begin();
    if (rc != MPI_SUCCESS) return rc;
    // in place, recvbuf still holds the input later rounds push: results via hold
    char* out = b.in_place ? b.hold : (bd.place == Place::Device ? static_cast<char*>(bd.dev) : w.out(me));
    const bool out_window = !b.in_place && out == w.out(me);   // host recvbuf: round by round via OUT
    const size_t nrounds = b.maxcnt ? (b.maxcnt + qh_el - 1) / qh_el : 1;
    unsigned long long seq = 0;
    std::vector<char*> subs((size_t)p);
    for (size_t ri = 0; ri < nrounds && rc == MPI_SUCCESS; ++ri) {
        const size_t o = ri * qh_el;
        const size_t half = (size_t)tp->rd_parity * half_bytes(p);
        seq = fc.seq();
        rc = fc.half_free(ri, seq, rc);
        Segs sg;
        std::vector<unsigned long long*> fl;
        for (int r = 0; r < p && rc == MPI_SUCCESS; ++r) {
            const size_t len = o < b.cnt(r) ? std::min(qh_el, b.cnt(r) - o) : 0;
            const char* v = nullptr;
            if (len)
                rc = device_view(bs, src, (b.disp[r] + o) * esz, len * esz,
                                 stage ? stage + (b.disp[r] + o) * esz : nullptr, s, &v);
            if (r == me) { subs[(size_t)me] = const_cast<char*>(v); continue; }
            subs[(size_t)r] = w.sub(me, r) + half;
            if (len && rc == MPI_SUCCESS) {
                sg.add(v, w.sub(r, me) + half, len * esz);
                if (!fault_drop_flags(me, seq)) fl.push_back(w.flags(r) + me);
            }
        }
        const size_t mylen = o < b.mycnt ? std::min(qh_el, b.mycnt - o) : 0;
        if (rc == MPI_SUCCESS) rc = fc.push(sg, fl, seq, mylen ? p : 0, "reduce_scatter push");
        if (rc == MPI_SUCCESS && mylen) {
            char* ro = out_window ? out : out + o * esz;
            rc = run_rank_tree(opidx, k, t, subs, esz, 0, mylen, ro, s);
            if (rc == MPI_SUCCESS && out_window) rc = copy_async(dst + o * esz, ro, mylen * esz, s);
        }
        // this round's half is read: free two rounds on
        if (rc == MPI_SUCCESS && ri + 2 < nrounds) rc = fc.post_half_done(seq);
        tp->rd_parity ^= 1;
    }
    if (rc == MPI_SUCCESS && b.mycnt && b.in_place) rc = copy_async(dst, out, b.mycnt * esz, s);
    ++g_stats.flag_calls;
    rc = fc.finish(rc, seq, "reduce_scatter one-step", "reduce_scatter");
    trace("reduce_scatter: done (GPU flags, %zu round(s), last seq %llu) rc=%d", nrounds, seq, rc);
    return rc;
}

// Host-barrier rounds of qe elements per block; `stage` holds the p pieces of
// one round of a host-resident input.
int Call::reduce_scatter_barrier(const RankTree& t, const RsBlocks& b, size_t qe) const
{
    std::vector<char*> subs = in_subs();
    int rc = MPI_SUCCESS;
    for (size_t o = 0; o < b.maxcnt && rc == MPI_SUCCESS; o += qe) {
        // my contribution to every destination's block range [o, o+qe)
        Segs scatter;
        for (int r = 0; r < p && rc == MPI_SUCCESS; ++r) {
            if (o >= b.cnt(r)) continue;
            const size_t len = std::min(qe, b.cnt(r) - o);
            const char* v = nullptr;
            rc = device_view(bs, src, (b.disp[r] + o) * esz, len * esz, stage ? stage + (size_t)r * qe * esz : nullptr,
                             s, &v);
            if (r == me) subs[(size_t)me] = const_cast<char*>(v);   // read in place
            else scatter.add(v, w.sub(r, me), len * esz);
        }
        if (rc == MPI_SUCCESS) rc = scatter.run(s, "reduce_scatter scatter");
        if (rc == MPI_SUCCESS) rc = sync_stream(s, "reduce_scatter scatter");
        if (rc == MPI_SUCCESS) rc = tp->barrier();                                  // A
        if (rc != MPI_SUCCESS) break;
        if (o < b.mycnt) {
            const size_t len = std::min(qe, b.mycnt - o);
            // In place, recvbuf is still our input for later rounds: results go
            // to a private device scratch and are copied out at the end.
            char* out = b.in_place ? b.hold + o * esz
                                   : (bd.place == Place::Device ? static_cast<char*>(bd.dev) + o * esz : w.out(me));
            rc = run_rank_tree(opidx, k, t, subs, esz, 0, len, out, s);
            if (rc == MPI_SUCCESS && out == w.out(me)) rc = copy_async(dst + o * esz, out, len * esz, s);
            if (rc == MPI_SUCCESS) rc = sync_stream(s, "reduce_scatter reduce");
        }
        if (rc == MPI_SUCCESS) rc = tp->barrier();                                  // B
    }
    if (rc == MPI_SUCCESS && b.in_place && b.mycnt) {
        rc = copy_async(dst, b.hold, b.mycnt * esz, s);
        if (rc == MPI_SUCCESS) rc = sync_stream(s, "reduce_scatter result");
    }
    trace("reduce_scatter: done rc=%d", rc);
    return rc;
}

int do_reduce_scatter(Comm* comm, const void* sendbuf, void* recvbuf, const int* recvcounts,
                      MPI_Datatype dt, const OpRef& op)
{
    if (op.dev_fn) return devop_reduce_scatter(comm, sendbuf, recvbuf, recvcounts, dt, op);
    Transport* tp = comm->tp;
    const int p = comm->size, me = comm->rank;
    const size_t esz = dtype_is_derived(dt) ? 0 : (size_t)type_size(dt);   // derived: user ops only
    RsBlocks b{recvcounts, std::vector<size_t>((size_t)p + 1, 0)};
    for (int r = 0; r < p; ++r) {
        b.disp[r + 1] = b.disp[r] + b.cnt(r);
        b.maxcnt = std::max(b.maxcnt, b.cnt(r));
    }
    const size_t total = b.total = b.disp[p];
    if (total == 0) return MPI_SUCCESS;
    b.mycnt = b.cnt(me);
    b.in_place = (sendbuf == MPI_IN_PLACE);
    const char* src = static_cast<const char*>(b.in_place ? recvbuf : sendbuf);
    if (op.opidx == O_NULL) return host_user_reduce_scatter(comm, src, recvbuf, b, dt, op);
    int rc = ensure_device();
    if (rc != MPI_SUCCESS) return rc;
    if (rccl_requested())
        if (ncclComm_t rcomm = rccl_comm(tp)) return rccl_reduce_scatter(rcomm, comm, sendbuf, recvbuf, recvcounts, dt, op);
    Call c{tp, p, me, op.opidx, type_info(dt)->kind, esz, tp->stream(), src, static_cast<char*>(recvbuf)};
    // GPU-synchronised rounds (decided by recvcounts, type, p and the
    // environment: the same on every rank): in round k, slice k of block r of
    // my input (at most half an IN sub-slot) goes into rank r's IN half with
    // its arrival flag while one workgroup waits for the peers' slices of my
    // block (k_push_wait), then my slice is evaluated.  One round when every
    // block fits half a sub-slot; longer blocks (c4: 512 MiB per rank at
    // p = 8) pipeline their rounds with GPU "half free" flags as the two-step
    // allreduce does, one host sync per call instead of four per round.
    const size_t qh_el = esz ? granules(half_bytes(p), esz) : 0;
    const bool one_step = p >= 2 && p <= 32 && tp->has_done() && total * esz <= two_step_max(tp) && qh_el > 0;
    if ((rc = get_windows(tp, &c.w, one_step)) != MPI_SUCCESS) return rc;
    // sub-slot k of IN(r) receives rank k's contribution to r's block, qe
    // elements per round
    const size_t qe = granules(c.w.Q, esz);
    if (qe == 0) { set_error("reduce_scatter: window too small"); return MPI_ERR_INTERN; }
    const int algo = reduce_scatter_algo(p, total, gate_type_size(dt, false), op.commutative);
    const RankTree t = rs_tree(algo, p, me);
    trace("reduce_scatter: total=%zu esz=%zu algo=%d round=%zu", total, esz, algo, qe);
    PinHold pins;
    c.alias_operands(pins, total * esz, b.in_place ? nullptr : recvbuf, b.in_place ? 0 : b.mycnt * esz);
    // scratch: [hold: in-place results][stage: host-resident input pieces --
    // the whole input for the flag rounds, one round's p pieces otherwise]
    const size_t hold_b = b.in_place ? up256(b.mycnt * esz) : 0;
    const size_t stage_b = c.bs.place == Place::Device ? 0 : (one_step ? total : (size_t)p * qe) * esz;
    if (hold_b + stage_b) {
        b.hold = dev_scratch(hold_b + stage_b);
        if (!b.hold) { set_error("reduce_scatter: scratch allocation failed"); return MPI_ERR_NO_MEM; }
        c.stage = b.hold + hold_b;
    }
    return one_step ? c.reduce_scatter_flags(t, b, qh_el) : c.reduce_scatter_barrier(t, b, qe);
}

// ---- scan / exscan ----------------------------------------------------------

int combine2(int opidx, Kind k, const char* inout_src, const char* in, char* out, size_t n, hipStream_t s,
             char* out2 = nullptr)
{
    TreeSpec t;
    t.P = 2;
    t.src[0] = inout_src;
    t.src[2] = in;
    if (out2) {                          // the same result stored twice
        t.extra[0] = out2;
        t.nextra = 1;
    }
    return hip_rc(launch_tree_spec(opidx, k, t, out, n, s), "scan combine");
}

// Flag steps: the vector fits half an IN sub-slot.  `stage` holds four blocks
// of up256(bytes): partial, result, and the two host operands.
int Call::scan_flags(size_t count, bool exclusive) const
{
    // Every step on the stream, one host sync: step i = one k_push_wait
    // (my partial -> IN(me ^ mask) half, sub-slot me, flag (seq << 6) | i;
    // one workgroup waits for the partial I consume), then the combines.
    // Halves alternate and are reused as in the two-step allreduce.
    // Launches are kept to the minimum (each costs a few us on its own GPU
    // and tens of us when ranks share one): step 0 reads the send buffer
    // in place; while partial and result hold the same value (inclusive
    // scan until this rank first folds a higher rank's partial) one
    // combine stores both; the last step stores the result straight into
    // recvbuf and drops the partial nobody reads again.
    const size_t bytes = count * esz, bstride = up256(bytes);
    char *partial = stage, *res = partial + bstride;
    char *src_stage = res + bstride, *dst_stage = src_stage + bstride;   // host operands the kernels cannot address
    const size_t half = (size_t)tp->rd_parity * half_bytes(p);
    FlagCall fc{*this, "scan"};
    const unsigned long long seq = fc.seq();
    int rc = fc.begin();
    if (rc != MPI_SUCCESS) return rc;
    // the kernels read the send buffer and write recvbuf in place when
    // they are device memory (or pinned aliases); host memory is staged
    const bool src_dev = bs.place == Place::Device, dst_dev = bd.place == Place::Device;
    const char* sv = srcv();
    if (!src_dev) {
        rc = copy_async(src_stage, src, bytes, s);
        sv = src_stage;
    }
    bool have = !exclusive;
    const char* cur_p = sv;                         // current partial
    const char* cur_r = exclusive ? nullptr : sv;   // current result (have)
    bool same = !exclusive;                         // partial and result hold one value
    char* outv = dst_dev ? dstv() : dst_stage;
    int step = 0;
    for (int mask = 1; mask < p && rc == MPI_SUCCESS; mask <<= 1, ++step) {
        const int dst = me ^ mask;
        const bool last = (mask << 1) >= p;
        const bool use = dst < p && !(last && me < dst);
        const bool feeds = dst < p && !(last && dst < me);
        const unsigned long long v = (seq << 6) | (unsigned long long)step;
        if (feeds && seq > 2) rc = tp->wait_done(dst, seq - 2);
        if (rc != MPI_SUCCESS) break;
        const void* ps = cur_p;
        void* pd = feeds ? static_cast<void*>(w.sub(dst, me) + half) : nullptr;
        size_t pn = bytes;
        unsigned long long* pf = feeds ? w.flags(dst) + kScanFlags + me : nullptr;
        hipError_t e = launch_push_wait(&ps, &pd, &pn, feeds ? 1 : 0, &pf, feeds ? 1 : 0, v,
                                        fc.counter + kCountWords,
                                        use ? w.flags(me) + kScanFlags + dst : w.flags(me), use ? 1 : 0, -1,
                                        fc.err_dev, s);
        if (e != hipSuccess) { rc = hip_fail(e, "scan push"); break; }
        if (!use) continue;
        const char* tmp = w.sub(me, dst) + half;
        // the partial is read again only by a later step's push or combine
        char* np = last ? nullptr : partial;
        if (me > dst) {
            char* nr = last ? outv : res;
            if (have && same) {                      // one combine, stored twice
                rc = np ? combine2(opidx, k, cur_p, tmp, np, count, s, nr)
                        : combine2(opidx, k, cur_r, tmp, nr, count, s);
            } else {
                if (np) rc = combine2(opidx, k, cur_p, tmp, np, count, s);
                if (rc == MPI_SUCCESS)
                    rc = have ? combine2(opidx, k, cur_r, tmp, nr, count, s) : copy_async(nr, tmp, bytes, s);
                same = false;
            }
            cur_p = np;
            cur_r = nr;
            have = true;
        } else {                                     // never the last step (use)
            rc = combine2(opidx, k, cur_p, tmp, partial, count, s);
            cur_p = partial;
            same = false;
        }
    }
    // a result that never left the send buffer or the scratch (rank 0 of an
    // inclusive scan, or a last step that did not fold) goes to recvbuf
    if (rc == MPI_SUCCESS && have && (cur_r != outv || !dst_dev))
        rc = copy_async(dst_dev ? outv : this->dst, cur_r, bytes, s);
    rc = fc.finish(rc, seq, "scan", "scan", false);
    tp->rd_parity ^= 1;
    return rc;
}

// Host-barrier steps, ce elements at a time through the halves of the IN area.
int Call::scan_barrier(size_t count, bool exclusive, size_t ce) const
{
    const size_t bytes = count * esz;
    char *partial = stage, *res = partial + up256(bytes);
    bool have = !exclusive;
    int rc = copy_async(partial, srcv(), bytes, s);
    if (rc == MPI_SUCCESS && !exclusive) rc = copy_async(res, srcv(), bytes, s);
    if (rc == MPI_SUCCESS) rc = sync_stream(s, "scan init");
    int slot = 0;
    for (int mask = 1; mask < p && rc == MPI_SUCCESS; mask <<= 1) {
        const int dst = me ^ mask;
        const bool last = (mask << 1) >= p;
        const bool use = dst < p && !(last && me < dst);     // this rank consumes dst's partial
        const bool feeds = dst < p && !(last && dst < me);   // dst consumes this rank's partial
        for (size_t o = 0; o < count && rc == MPI_SUCCESS; o += ce, slot ^= 1) {
            const size_t len = std::min(ce, count - o);
            if (feeds) {
                char* peer_in = w.in(dst) + (size_t)slot * (w.C / 2);
                rc = copy_async(peer_in, partial + o * esz, len * esz, s);   // partial at step start
                if (rc == MPI_SUCCESS) rc = sync_stream(s, "scan push");
            }
            if (rc == MPI_SUCCESS) rc = tp->barrier();
            if (rc != MPI_SUCCESS || !use) continue;
            const char* tmp = w.in(me) + (size_t)slot * (w.C / 2);
            char* pp = partial + o * esz;
            char* rr = res + o * esz;
            if (me > dst) {
                rc = combine2(opidx, k, pp, tmp, pp, len, s);
                if (rc == MPI_SUCCESS)
                    rc = have ? combine2(opidx, k, rr, tmp, rr, len, s) : copy_async(rr, tmp, len * esz, s);
            } else {
                rc = combine2(opidx, k, pp, tmp, pp, len, s);             // builtins commute
            }
            if (rc == MPI_SUCCESS) rc = sync_stream(s, "scan step");
        }
        if (use && me > dst) have = true;
    }
    if (rc == MPI_SUCCESS) rc = tp->barrier();
    if (rc == MPI_SUCCESS && have) {
        rc = copy_async(dstv(), res, bytes, s);
        if (rc == MPI_SUCCESS) rc = sync_stream(s, "scan result");
    }
    return rc;
}

int do_scan(Comm* comm, const void* sendbuf, void* recvbuf, size_t count, MPI_Datatype dt,
            const OpRef& op, bool exclusive)
{
    if (op.dev_fn) return devop_scan(comm, sendbuf, recvbuf, count, dt, op, exclusive);
    if (op.opidx == O_NULL) return host_user_scan(comm, sendbuf, recvbuf, count, dt, op, exclusive);
    int rc = ensure_device();
    if (rc != MPI_SUCCESS) return rc;
    Transport* tp = comm->tp;
    const int p = comm->size;
    const size_t esz = (size_t)type_info(dt)->size, bytes = count * esz;
    Call c{tp, p, comm->rank, op.opidx, type_info(dt)->kind, esz, tp->stream(),
           static_cast<const char*>(sendbuf == MPI_IN_PLACE ? recvbuf : sendbuf), static_cast<char*>(recvbuf)};
    // GPU-synchronised when the vector fits half an IN sub-slot (count, type,
    // p and the environment decide: the same on every rank)
    const bool flags = p >= 2 && p <= 32 && tp->has_done() && bytes <= half_bytes(p) && bytes <= two_step_max(tp);
    if ((rc = get_windows(tp, &c.w, flags)) != MPI_SUCCESS) return rc;
    // Each step's partial is PUSHED into the consumer's IN window (an xGMI
    // remote write) and combined there from local HBM; two alternating halves
    // of IN: a peer writes step i+2's half only after the barrier of step i+1,
    // which this rank reaches after finishing its reads of step i.
    const size_t ce = granules(c.w.C / 2, esz);
    if (ce == 0) { set_error("scan: window too small"); return MPI_ERR_INTERN; }
    c.stage = dev_scratch(4 * up256(bytes) + 256);
    if (!c.stage) { set_error("scan: scratch allocation failed"); return MPI_ERR_NO_MEM; }
    PinHold pins;
    c.alias_operands(pins, bytes, recvbuf, bytes);
    return flags ? c.scan_flags(count, exclusive) : c.scan_barrier(count, exclusive, ce);
}

}  // namespace

// ---- public engine entry points --------------------------------------------
int engine_allreduce(Comm* c, const void* sendbuf, void* recvbuf, size_t count, MPI_Datatype dt,
                     const OpRef& op, bool nbc)
{
    return worker().run([=] { return do_allreduce(c, sendbuf, recvbuf, count, dt, op, -1, nbc); });
}

int engine_reduce_scatter(Comm* c, const void* sendbuf, void* recvbuf, const int* recvcounts,
                          MPI_Datatype dt, const OpRef& op)
{
    std::vector<int> counts(recvcounts, recvcounts + c->size);
    return worker().run([=] { return do_reduce_scatter(c, sendbuf, recvbuf, counts.data(), dt, op); });
}

int engine_reduce(Comm* c, const void* sendbuf, void* recvbuf, size_t count, MPI_Datatype dt,
                  const OpRef& op, int root, bool nbc)
{
    // Builtin ops: the reference's binomial / Rabenseifner trees (do_allreduce
    // in reduce mode); user ops: host_user_reduce.
    return worker().run([=]() -> int {
        if (op.dev_fn) return devop_reduce(c, sendbuf, recvbuf, count, dt, op, root);
        if (op.opidx == O_NULL) return host_user_reduce(c, sendbuf, recvbuf, count, dt, op, root);
        return do_allreduce(c, sendbuf, recvbuf, count, dt, op, root, nbc);
    });
}

int engine_scan(Comm* c, const void* sendbuf, void* recvbuf, size_t count, MPI_Datatype dt,
                const OpRef& op, bool exclusive)
{
    return worker().run([=] { return do_scan(c, sendbuf, recvbuf, count, dt, op, exclusive); });
}

}  // namespace msx
