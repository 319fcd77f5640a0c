// msx_collectives.cpp — the collective schedules over the engine windows:
// the two-step chunk plan, allreduce / reduce, reduce_scatter, scan / exscan
// and their public engine_* entry points.
#include "msx_engine.h"

#include <algorithm>
#include <string.h>

namespace msx {

// Elements per chunk of the pipelined two-step allreduce / reduce for p ranks
// and elements of esz bytes: p pieces of at most half an IN sub-slot each, the
// whole chunk within half the OUT area above the recursive-doubling results,
// whole 16-element pieces (0: the window is too small).
size_t two_step_chunk_el(int p, size_t esz)
{
    const size_t Qh = (sub_len(chunk_bytes(), p) / 2) & ~(size_t)255;
    const size_t qh_el = (Qh / esz) & ~(size_t)15;
    const size_t out_half = ((chunk_bytes() - Qh) / 2) & ~(size_t)255;
    size_t pc_el = std::min((size_t)p * qh_el, out_half / esz);
    return pc_el - pc_el % ((size_t)p * 16);
}

// Rank me's part of chunk ci: its piece [plo, phi) of the chunk (16-element
// granules) cut where the owner tree changes -- the owner of an element is
// that of its block in the WHOLE vector (allreduce_block, reduce.cpp:3927-
// 4066), so the chunking never changes a result.  Offsets are relative to
// the chunk start o = ci * pc_el.
void two_step_plan(int p, size_t count, size_t pc_el, size_t ci, int me, std::vector<TwoStepRange>* ranges,
                   size_t* plo, size_t* phi, size_t* len_out)
{
    const int pof2 = pof2_floor(p);
    const size_t o = ci * pc_el, len = std::min(pc_el, count - o);
    const size_t pel = (((len + (size_t)p - 1) / (size_t)p) + 15) & ~(size_t)15;
    *plo = std::min(len, (size_t)me * pel);
    *phi = std::min(len, (size_t)(me + 1) * pel);
    *len_out = len;
    ranges->clear();
    const size_t rs = count / (size_t)pof2;
    for (size_t e0 = *plo; e0 < *phi;) {
        const size_t ge = o + e0;
        const int j = rs ? (int)std::min((size_t)pof2 - 1, ge / rs) : pof2 - 1;
        size_t bst, bl;
        allreduce_block(p, count, j, &bst, &bl);
        const size_t e1 = std::min(*phi, bst + bl - o);
        ranges->push_back({e0, e1, allreduce_block_owner(p, j)});
        e0 = e1;
    }
}

// root < 0: allreduce; root >= 0: only `root` receives the result (MPI_Reduce).
int do_allreduce(Comm* c, const void* sendbuf, void* recvbuf, size_t count, MPI_Datatype dt,
                 const OpRef& op, int root, bool nbc)
{
    // device user ops stay in HBM (msx_devop.cpp); MPI_Op_create's functions
    // are host code: no GPU needed on that path
    if (op.dev_fn) return devop_allreduce(c, sendbuf, recvbuf, count, dt, op);
    if (op.opidx == O_NULL) return host_user_allreduce(c, sendbuf, recvbuf, count, dt, op);
    int rc = ensure_device();
    if (rc != MPI_SUCCESS) return rc;

    Transport* tp = c->tp;
    if (rccl_requested())
        if (ncclComm_t rcomm = rccl_comm(tp)) return rccl_allreduce(rcomm, c, sendbuf, recvbuf, count, dt, op, root, nbc);
    const int p = c->size, me = c->rank;
    const TypeInfo* ti = type_info(dt);
    const Kind k = ti->kind;
    const size_t esz = (size_t)ti->size;
    hipStream_t s = tp->stream();
    const char* src = static_cast<const char*>(sendbuf == MPI_IN_PLACE ? recvbuf : sendbuf);
    char* dst = static_cast<char*>(recvbuf);
    const bool want = (root < 0 || root == me);          // this rank receives the result
    const bool is_reduce = root >= 0;
    const int gate = gate_type_size(dt, nbc);
    const int algo = is_reduce ? reduce_algo(p, count, gate, true) : allreduce_algo(p, count, gate, true);
    // A recursive-doubling (or binomial) call that fits half a sub-slot runs
    // barrier-free at its end: it uses the IN half `rd_parity`, alternating per
    // call.  Pushing into a peer's half P again (two calls later) happens only
    // after this rank passed the previous call's barrier A, which that peer
    // reached only after finishing its tree on half P.
    const size_t Qh = (sub_len(chunk_bytes(), p) / 2) & ~(size_t)255;
    const bool rd_single = (algo == A_RECURSIVE_DOUBLING || algo == A_BINOMIAL) &&
                           count * esz <= (Qh & ~(size_t)(16 * esz - 1)) && p <= 32 && tp->has_done();
    // Rabenseifner in two GPU-synchronised steps per chunk (see below): a
    // chunk is p pieces of at most half an IN sub-slot each and fits half the
    // OUT area above the recursive-doubling results; a longer message runs as
    // a pipeline of such chunks.  Only count, type, p and the environment
    // decide, so every rank takes the same branch and the same chunks.
    const size_t out_half = ((chunk_bytes() - Qh) / 2) & ~(size_t)255;
    const size_t pc_el = two_step_chunk_el(p, esz);
    const bool two_step = algo == A_RABENSEIFNER && p >= 2 && p <= 32 && tp->has_done() &&
                          count * esz <= two_step_max(tp) && pc_el > 0;
    Windows w;
    if ((rc = get_windows(tp, &w, rd_single || two_step)) != MPI_SUCCESS) return rc;
    // host buffers: device aliases for the call (pinned in place of staging)
    BufInfo bs = classify(src), bd = classify(dst);
    PinHold pins;
    pins.sync_before_release(s);
    if (hipStream_t a = aux_stream(tp)) pins.sync_before_release(a);
    alias_host_operands(pins, true, src, count * esz, &bs, want ? dst : nullptr, want ? count * esz : 0, &bd);
    // elements per sub-slot, whole 16-element granules
    size_t qmax = w.Q / esz;
    qmax -= qmax % 16;
    if (qmax == 0) { set_error("allreduce: window too small"); return MPI_ERR_INTERN; }
    char* stage = nullptr;
    if (bs.place != Place::Device) {
        stage = dev_scratch(std::min(count, (size_t)p * qmax) * esz);
        if (!stage) { set_error("allreduce: scratch allocation failed"); return MPI_ERR_NO_MEM; }
    }
    const int pof2 = pof2_floor(p);
    const int n = newrank_of(me, p);
    const int lineage = n >= 0 ? n : newrank_of(me + 1, p);
    std::vector<char*> subs((size_t)p);
    for (int r = 0; r < p; ++r) subs[r] = w.sub(me, r);
    trace("allreduce: count=%zu esz=%zu algo=%d qmax=%zu", count, esz, algo, qmax);

    if (algo == A_RECURSIVE_DOUBLING || algo == A_BINOMIAL) {
        // every rank that evaluates a tree needs every contribution whole:
        // recursive doubling -> all ranks evaluate their own lineage's tree;
        // binomial reduce -> only the root evaluates
        const RankTree t = (algo == A_BINOMIAL) ? tree_reduce_binomial(p, root) : tree_allreduce(p, lineage);
        if (rd_single) {
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
            const size_t half = (size_t)tp->rd_parity * Qh;
            for (int r = 0; r < p; ++r) subs[r] = w.sub(me, r) + half;
            // small host buffers go through the engine's pinned bounce buffers
            // (CPU copies in and out, the kernels read / write them over PCIe)
            // instead of synchronous pageable copies through HBM staging
            const size_t nbytes = count * esz;
            const bool bounce_src = bs.place != Place::Device && nbytes <= bounce_max_bytes() &&
                                    engine_bounce(0).get(nbytes);
            const bool bounce_dst = want && bd.place != Place::Device && nbytes <= bounce_max_bytes() &&
                                    engine_bounce(1).get(nbytes);
            const char* mine = nullptr;
            if (bounce_src) {
                memcpy(engine_bounce(0).host, src, nbytes);
                mine = engine_bounce(0).dev;
            } else {
                rc = device_view(bs, src, 0, nbytes, stage, s, &mine);
            }
            const unsigned long long seq = ++tp->rd_seq;
            Segs sg;
            std::vector<unsigned long long*> fl;
            for (int r = 0; r < p && rc == MPI_SUCCESS; ++r)
                if (r != me && (root < 0 || r == root)) {
                    if (seq > 2) rc = tp->wait_done(r, seq - 2);
                    sg.add(mine, w.sub(r, me) + half, count * esz);
                    if (!fault_drop_flags(me, seq)) fl.push_back(w.flags(r) + me);
                }
            subs[(size_t)me] = const_cast<char*>(mine);
            int* err_host = nullptr;
            int* err_dev = wait_err_word(&err_host);
            if (!err_dev) { set_error("allreduce: arrival word allocation failed"); return MPI_ERR_NO_MEM; }
            *err_host = 0;
            char* out = bd.place == Place::Device ? static_cast<char*>(bd.dev)
                                                  : (bounce_dst ? engine_bounce(1).dev : w.out(me));
            unsigned* counter = nullptr;
            if (rc == MPI_SUCCESS && !sg.src.empty()) {
                counter = tp->push_counter();
                if (!counter) { set_error("allreduce: push counter allocation failed"); return MPI_ERR_NO_MEM; }
            }
            if (rc == MPI_SUCCESS) {
                hipError_t e = launch_push_wait(sg.src.data(), sg.dst.data(), sg.n.data(), (int)sg.src.size(),
                                                fl.data(), (int)fl.size(), seq,
                                                counter ? counter + kCountWords : nullptr, w.flags(me),
                                                want ? p : 0, me, err_dev, s);
                if (e != hipSuccess) rc = hip_fail(e, "allreduce push");
            }
            if (rc == MPI_SUCCESS && want) {
                rc = run_rank_tree(op.opidx, k, t, subs, esz, 0, count, out, s);   // after the wait, in stream order
                if (rc == MPI_SUCCESS && out == w.out(me)) rc = copy_async(dst, out, count * esz, s);
            }
            const int rs = sync_stream(s, "allreduce tree");
            if (rc == MPI_SUCCESS) rc = rs;
            if (rc == MPI_SUCCESS && bounce_dst) memcpy(dst, engine_bounce(1).host, nbytes);
            if (rc == MPI_SUCCESS && __atomic_load_n(err_host, __ATOMIC_ACQUIRE))
                rc = flag_timeout(root < 0 ? "allreduce" : "reduce", me, __atomic_load_n(err_host, __ATOMIC_ACQUIRE),
                                  seq);
            tp->post_done(seq);                   // this rank's tree no longer reads the half
            tp->rd_parity ^= 1;
            tp->window_open = true;
            trace("allreduce: done (GPU arrival flags, seq %llu) rc=%d", seq, rc);
            return rc;
        }
        for (size_t o = 0; o < count && rc == MPI_SUCCESS; o += qmax) {
            const size_t len = std::min(qmax, count - o);
            const char* mine = nullptr;
            rc = device_view(bs, src, o * esz, len * esz, stage, s, &mine);
            Segs sg;                      // my own contribution is read in place
            for (int r = 0; r < p; ++r)
                if (r != me && (root < 0 || r == root)) sg.add(mine, w.sub(r, me), len * esz);
            subs[(size_t)me] = const_cast<char*>(mine);
            if (rc == MPI_SUCCESS) rc = sg.run(s, "allreduce push");
            if (rc == MPI_SUCCESS) rc = sync_stream(s, "allreduce push");
            if (rc == MPI_SUCCESS) rc = tp->barrier();                              // A
            if (rc == MPI_SUCCESS && want) {
                char* out = bd.place == Place::Device ? static_cast<char*>(bd.dev) + o * esz : w.out(me);
                rc = run_rank_tree(op.opidx, k, t, subs, esz, 0, len, out, s);
                if (rc == MPI_SUCCESS && out == w.out(me)) rc = copy_async(dst + o * esz, out, len * esz, s);
                if (rc == MPI_SUCCESS) rc = sync_stream(s, "allreduce tree");
            }
            if (rc == MPI_SUCCESS) rc = tp->barrier();                              // B
        }
        trace("allreduce: done rc=%d", rc);
        return rc;
    }

    if (two_step) {
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
        if (!tp->out_quiet && (rc = tp->barrier()) != MPI_SUCCESS) return rc;
        int* err_host = nullptr;
        int* err_dev = wait_err_word(&err_host);
        unsigned* counter = tp->push_counter();
        if (!err_dev || !counter) { set_error("allreduce: flag word allocation failed"); return MPI_ERR_NO_MEM; }
        *err_host = 0;
        std::vector<int> dests;
        if (want) dests.push_back(me);
        for (int r = 0; r < p; ++r)
            if (r != me && (root < 0 || r == root)) dests.push_back(r);
        std::vector<unsigned long long*> done_to;            // my GPU done flag in every peer's window
        for (int r = 0; r < p; ++r)
            if (r != me) done_to.push_back(w.flags(r) + kDoneFlags + me);
        const size_t nchunks = (count + pc_el - 1) / pc_el;
        unsigned long long seq = 0;
        size_t nranges = 0;
        std::vector<TwoStepRange> ranges;
        for (size_t ci = 0; ci < nchunks && rc == MPI_SUCCESS; ++ci) {
            const size_t o = ci * pc_el;
            size_t plo, phi, len;
            two_step_plan(p, count, pc_el, ci, me, &ranges, &plo, &phi, &len);
            const size_t pel = (((len + (size_t)p - 1) / (size_t)p) + 15) & ~(size_t)15;
            auto lo_of = [&](int r) { return std::min(len, (size_t)r * pel); };
            auto hi_of = [&](int r) { return std::min(len, (size_t)(r + 1) * pel); };
            const size_t half = (size_t)tp->rd_parity * Qh;
            const size_t obase = Qh + (size_t)tp->rd_parity * out_half;
            const char* mine = nullptr;
            rc = device_view(bs, src, o * esz, len * esz, stage, s, &mine);
            seq = ++tp->rd_seq;
            if (ci < 2) {
                for (int r = 0; r < p && rc == MPI_SUCCESS; ++r)
                    if (r != me && seq > 2) rc = tp->wait_done(r, seq - 2);
            } else if (rc == MPI_SUCCESS) {
                hipError_t e = launch_push_wait(nullptr, nullptr, nullptr, 0, nullptr, 0, seq - 2, nullptr,
                                                w.flags(me) + kDoneFlags, p, me, err_dev, s, 3);
                if (e != hipSuccess) rc = hip_fail(e, "allreduce half-free wait");
            }
            if (rc != MPI_SUCCESS) break;
            Segs sg;
            std::vector<unsigned long long*> fl, done;
            for (int r = 0; r < p; ++r) {
                if (r == me || hi_of(r) <= lo_of(r)) continue;
                sg.add(mine + lo_of(r) * esz, w.sub(r, me) + half, (hi_of(r) - lo_of(r)) * esz);
                if (!fault_drop_flags(me, seq)) fl.push_back(w.flags(r) + me);
            }
            for (int d : dests)
                if (d != me) done.push_back(w.flags(d) + kResultFlags + me);
            nranges += ranges.size();
            for (int r = 0; r < p; ++r) subs[r] = w.sub(me, r) + half;
            subs[(size_t)me] = const_cast<char*>(mine) + plo * esz;
            // step 1: push my pieces and their arrival flags; one workgroup
            // waits for the peers' pieces of mine (none when my piece is empty)
            hipError_t e = launch_push_wait(sg.src.data(), sg.dst.data(), sg.n.data(), (int)sg.src.size(), fl.data(),
                                            (int)fl.size(), seq, counter + kCountWords, w.flags(me),
                                            ranges.empty() ? 0 : p, me, err_dev, s);
            if (e != hipSuccess) rc = hip_fail(e, "allreduce push");
            // step 2: my piece into every receiver's OUT half; the last
            // workgroup of the last launch posts the result flags
            if (rc == MPI_SUCCESS && ranges.empty() && !done.empty()) {
                e = launch_post_flags(done.data(), (int)done.size(), seq, s);
                if (e != hipSuccess) rc = hip_fail(e, "allreduce result flags");
            }
            for (size_t i = 0; i < ranges.size() && rc == MPI_SUCCESS; ++i) {
                const TwoStepRange& g = ranges[i];
                const RankTree t = !is_reduce ? tree_allreduce(p, g.owner)
                                              : (nbc ? tree_ireduce_rsag(p, g.owner, root) : tree_reduce_rsag(p, g.owner));
                std::vector<char*> extra;
                for (size_t d = 1; d < dests.size(); ++d) extra.push_back(w.out(dests[d]) + obase + g.e0 * esz);
                TreeWait tw;
                tw.done_counter = counter + 2 * kCountWords;
                tw.done_launches = (unsigned)ranges.size();
                tw.done_flags = &done;
                tw.done_seq = seq;
                rc = run_rank_tree(op.opidx, k, t, subs, esz, g.e0 - plo, g.e1 - g.e0,
                                   w.out(dests[0]) + obase + g.e0 * esz, s, extra, &tw);
            }
            if (rc == MPI_SUCCESS && want) {
                // step 3: every peer's result in my OUT half, then into recvbuf
                e = launch_push_wait(nullptr, nullptr, nullptr, 0, nullptr, 0, seq, nullptr,
                                     w.flags(me) + kResultFlags, p, me, err_dev, s, 2);
                if (e != hipSuccess) rc = hip_fail(e, "allreduce result wait");
                char* out = bd.place == Place::Device ? static_cast<char*>(bd.dev) : dst;
                if (rc == MPI_SUCCESS) rc = copy_async(out + o * esz, w.out(me) + obase, len * esz, s);
            }
            // step 4: this chunk's halves are free again (read by my trees and
            // my copy, both earlier on the stream) -- only a later chunk of
            // this call waits on it
            if (rc == MPI_SUCCESS && ci + 2 < nchunks) {
                e = launch_post_flags(done_to.data(), (int)done_to.size(), seq, s);
                if (e != hipSuccess) rc = hip_fail(e, "allreduce done flags");
            }
            tp->rd_parity ^= 1;
        }
        ++g_stats.flag_calls;
        const int rsy = sync_stream(s, "allreduce two-step");
        if (rc == MPI_SUCCESS) rc = rsy;
        if (rc == MPI_SUCCESS && __atomic_load_n(err_host, __ATOMIC_ACQUIRE))
            rc = flag_timeout(root < 0 ? "allreduce" : "reduce", me, __atomic_load_n(err_host, __ATOMIC_ACQUIRE), seq);
        tp->post_done(seq);
        tp->window_open = true;
        tp->out_quiet = true;
        trace("allreduce: done (two-step, GPU flags, %zu chunk(s), last seq %llu, %zu ranges) rc=%d", nchunks, seq,
              nranges, rc);
        return rc;
    }

    // Rabenseifner order: element e belongs to block j(e), whose value the
    // reference computes at newrank bitrev(j).  Each chunk is cut into p
    // pieces (work balance only, 16-element granules); each element of a piece
    // is evaluated with the tree of its block's owner.
    const size_t ce = (size_t)p * qmax;
    hipStream_t s2 = aux_stream(tp) ? aux_stream(tp) : s;
    for (size_t o = 0; o < count && rc == MPI_SUCCESS; o += ce) {
        const double t0 = now_s();
        const size_t len = std::min(ce, count - o);
        const size_t q = (len + p - 1) / p;
        const size_t qv = (q + 15) & ~(size_t)15;
        auto lo_of = [&](int r) { return std::min(len, (size_t)r * qv); };
        auto hi_of = [&](int r) { return std::min(len, (size_t)(r + 1) * qv); };
        const char* mine = nullptr;
        rc = device_view(bs, src, o * esz, len * esz, stage, s, &mine);
        Segs scatter;
        for (int r = 0; r < p; ++r)                  // my own piece is read in place
            if (r != me) scatter.add(mine + lo_of(r) * esz, w.sub(r, me), (hi_of(r) - lo_of(r)) * esz);
        subs[(size_t)me] = const_cast<char*>(mine) + lo_of(me) * esz;
        if (rc == MPI_SUCCESS) rc = scatter.run(s, "allreduce scatter");
        if (rc == MPI_SUCCESS) rc = sync_stream(s, "allreduce scatter");
        const double t1 = now_s();
        if (rc == MPI_SUCCESS) rc = sync_stream(s2, "allreduce collect");           // OUT(me) free
        if (rc == MPI_SUCCESS) rc = tp->barrier();                                  // A
        const double t2 = now_s();
        if (rc != MPI_SUCCESS) break;
        const size_t plo = lo_of(me), phi = hi_of(me);
        // reduce my piece from my IN area (local) and store the result straight
        // into every receiver's OUT area: the push is fused into the tree
        // kernel (remote stores over xGMI)
        std::vector<int> dests;
        if (want) dests.push_back(me);
        for (int r = 0; r < p; ++r)
            if (r != me && (root < 0 || r == root)) dests.push_back(r);
        for (size_t e0 = plo; e0 < phi && rc == MPI_SUCCESS;) {
            const size_t ge = o + e0;                                             // global element
            const size_t rs = count / (size_t)pof2;
            const int j = rs ? (int)std::min((size_t)pof2 - 1, ge / rs) : pof2 - 1;
            size_t bst, bl;
            allreduce_block(p, count, j, &bst, &bl);
            const size_t e1 = std::min(phi, bst + bl - o);
            const int owner = allreduce_block_owner(p, j);
            const RankTree t = !is_reduce ? tree_allreduce(p, owner)
                                          : (nbc ? tree_ireduce_rsag(p, owner, root) : tree_reduce_rsag(p, owner));
            std::vector<char*> extra;
            for (size_t d = 1; d < dests.size(); ++d) extra.push_back(w.out(dests[d]) + e0 * esz);
            rc = run_rank_tree(op.opidx, k, t, subs, esz, e0 - plo, e1 - e0, w.out(dests[0]) + e0 * esz, s, extra);
            e0 = e1;
        }
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
        if (rc == MPI_SUCCESS && want) rc = copy_async(dst + o * esz, w.out(me), len * esz, s2);
    }
    const double tc = now_s();
    if (rc == MPI_SUCCESS) rc = sync_stream(s2, "allreduce collect");
    g_stats.t[4] += now_s() - tc;
    g_stats.calls += 1;
    trace("allreduce: done rc=%d", rc);
    return rc;
}

namespace {
int do_reduce_scatter(Comm* c, const void* sendbuf, void* recvbuf, const int* recvcounts,
                      MPI_Datatype dt, const OpRef& op)
{
    if (op.dev_fn) return devop_reduce_scatter(c, sendbuf, recvbuf, recvcounts, dt, op);
    Transport* tp = c->tp;
    const int p = c->size, me = c->rank;
    const size_t esz = dtype_is_derived(dt) ? 0 : (size_t)type_size(dt);   // derived: user ops only
    std::vector<size_t> disp((size_t)p + 1, 0);
    size_t maxcnt = 0;
    for (int r = 0; r < p; ++r) {
        disp[r + 1] = disp[r] + (size_t)recvcounts[r];
        maxcnt = std::max(maxcnt, (size_t)recvcounts[r]);
    }
    const size_t total = disp[p];
    if (total == 0) return MPI_SUCCESS;
    const bool in_place = (sendbuf == MPI_IN_PLACE);
    const char* src = static_cast<const char*>(in_place ? recvbuf : sendbuf);

    if (op.opidx == O_NULL) {
        // images of the whole input (total elements) and of my block (mycnt);
        // block r starts disp[r] elements (x extent for a derived type) into it
        const Img mf = img_of(dt, total), mb = img_of(dt, (size_t)recvcounts[me]);
        const int64_t unit = mf.t ? mf.t->extent : (int64_t)esz;
        std::vector<char> full(mf.bytes);
        int rc = img_load(mf, src, full.data());
        if (rc != MPI_SUCCESS) return rc;
        const size_t mycnt = (size_t)recvcounts[me];
        if (op.commutative) {
            // commutative user op: the builtin schedules (recursive halving or
            // pairwise, same 32-bit gate) evaluated on host with the user's
            // function, reduce.cpp:917-1334
            std::vector<char> all((size_t)p * mf.bytes);
            if ((rc = c->tp->allgather(full.data(), mf.bytes, all.data())) != MPI_SUCCESS) return rc;
            const int algo = reduce_scatter_algo(p, total, gate_type_size(dt, false), true);
            const int n = newrank_of(me, p);
            const RankTree t = (algo == A_RS_PAIRWISE) ? tree_pairwise(p, me)
                                                       : tree_reduce_scatter(p, n >= 0 ? n : newrank_of(me + 1, p));
            std::vector<const char*> x((size_t)p);
            for (int r = 0; r < p; ++r)
                x[(size_t)r] = all.data() + (size_t)r * mf.bytes - mf.lo + (int64_t)disp[me] * unit;
            std::vector<char> res(mb.bytes);
            eval_tree_host(t, x, res.data() - mb.lo, mycnt, dt, op, mb);
            return mycnt ? img_store(mb, mycnt, res.data() - mb.lo, recvbuf) : MPI_SUCCESS;
        }
        // non-commutative: recursive doubling (MPIR_Reduce_scatter_non_commutative,
        // reduce.cpp:1340-1630) -- for a power-of-two p each block is exactly the
        // recursive-doubling allreduce value; other p share its lower-first order
        std::vector<char> res(mf.bytes);
        rc = host_user_allreduce(c, full.data() - mf.lo, res.data() - mf.lo, total, dt, op);
        if (rc == MPI_SUCCESS && mycnt)
            rc = img_store(mb, mycnt, res.data() - mf.lo + (int64_t)disp[me] * unit, recvbuf);
        return rc;
    }
    int rc = ensure_device();
    if (rc != MPI_SUCCESS) return rc;
    if (rccl_requested())
        if (ncclComm_t rcomm = rccl_comm(tp)) return rccl_reduce_scatter(rcomm, c, sendbuf, recvbuf, recvcounts, dt, op);
    const Kind k = type_info(dt)->kind;
    hipStream_t s = tp->stream();
    // GPU-synchronised rounds (decided by recvcounts, type, p and the
    // environment: the same on every rank): in round k, slice k of block r of
    // my input (at most half an IN sub-slot) goes into rank r's IN half with
    // its arrival flag while one workgroup waits for the peers' slices of my
    // block (k_push_wait), then my slice is evaluated.  One round when every
    // block fits half a sub-slot; longer blocks (c4: 512 MiB per rank at
    // p = 8) pipeline their rounds with GPU "half free" flags as the two-step
    // allreduce does, one host sync per call instead of four per round.
    const size_t Qh = (sub_len(chunk_bytes(), p) / 2) & ~(size_t)255;
    const size_t qh_el = esz ? (Qh / esz) & ~(size_t)15 : 0;
    const bool one_step = p >= 2 && p <= 32 && tp->has_done() && total * esz <= two_step_max(tp) && qh_el > 0;
    Windows w;
    if ((rc = get_windows(tp, &w, one_step)) != MPI_SUCCESS) return rc;
    // sub-slot k of IN(r) receives rank k's contribution to r's block, qe
    // elements per round
    size_t qe = w.Q / esz;
    qe -= qe % 16;
    if (qe == 0) { set_error("reduce_scatter: window too small"); return MPI_ERR_INTERN; }
    const int algo = reduce_scatter_algo(p, total, gate_type_size(dt, false), op.commutative);
    const int n = newrank_of(me, p);
    const RankTree t = (algo == A_RS_PAIRWISE) ? tree_pairwise(p, me)
                                               : tree_reduce_scatter(p, n >= 0 ? n : newrank_of(me + 1, p));
    trace("reduce_scatter: total=%zu esz=%zu algo=%d round=%zu", total, esz, algo, qe);
    const size_t mycnt = (size_t)recvcounts[me];
    BufInfo bs = classify(src), bd = classify(recvbuf);
    PinHold pins;                        // host buffers: device aliases for the call
    pins.sync_before_release(s);
    alias_host_operands(pins, true, src, total * esz, &bs, in_place ? nullptr : recvbuf, in_place ? 0 : mycnt * esz,
                        &bd);
    char* dst = static_cast<char*>(recvbuf);
    if (one_step) {
        const size_t hold_b = in_place ? ((mycnt * esz + 255) & ~(size_t)255) : 0;
        const size_t stage_b = bs.place == Place::Device ? 0 : total * esz;
        char* scratch = nullptr;
        if (hold_b + stage_b) {
            scratch = dev_scratch(hold_b + stage_b);
            if (!scratch) { set_error("reduce_scatter: scratch allocation failed"); return MPI_ERR_NO_MEM; }
        }
        int* err_host = nullptr;
        int* err_dev = wait_err_word(&err_host);
        unsigned* counter = tp->push_counter();
        if (!err_dev || !counter) { set_error("reduce_scatter: flag word allocation failed"); return MPI_ERR_NO_MEM; }
        *err_host = 0;
        std::vector<unsigned long long*> done_to;          // my GPU done flag in every peer's window
        for (int r = 0; r < p; ++r)
            if (r != me) done_to.push_back(w.flags(r) + kDoneFlags + me);
        // in place, recvbuf still holds the input later rounds push: results via hold
        char* out = in_place ? scratch : (bd.place == Place::Device ? static_cast<char*>(bd.dev) : w.out(me));
        const bool out_window = !in_place && out == w.out(me);   // host recvbuf: round by round via OUT
        const size_t nrounds = maxcnt ? (maxcnt + qh_el - 1) / qh_el : 1;
        unsigned long long seq = 0;
        std::vector<char*> subs((size_t)p);
        for (size_t ri = 0; ri < nrounds && rc == MPI_SUCCESS; ++ri) {
            const size_t o = ri * qh_el;
            const size_t half = (size_t)tp->rd_parity * Qh;
            seq = ++tp->rd_seq;
            if (ri < 2) {
                for (int r = 0; r < p && rc == MPI_SUCCESS; ++r)
                    if (r != me && seq > 2) rc = tp->wait_done(r, seq - 2);
            } else if (rc == MPI_SUCCESS) {
                hipError_t e = launch_push_wait(nullptr, nullptr, nullptr, 0, nullptr, 0, seq - 2, nullptr,
                                                w.flags(me) + kDoneFlags, p, me, err_dev, s, 3);
                if (e != hipSuccess) rc = hip_fail(e, "reduce_scatter half-free wait");
            }
            Segs sg;
            std::vector<unsigned long long*> fl;
            for (int r = 0; r < p && rc == MPI_SUCCESS; ++r) {
                const size_t cnt = (size_t)recvcounts[r];
                const size_t len = o < cnt ? std::min(qh_el, cnt - o) : 0;
                const char* v = nullptr;
                if (len)
                    rc = device_view(bs, src, (disp[r] + o) * esz, len * esz,
                                     scratch ? scratch + hold_b + (disp[r] + o) * esz : nullptr, s, &v);
                if (r == me) { subs[(size_t)me] = const_cast<char*>(v); continue; }
                subs[(size_t)r] = w.sub(me, r) + half;
                if (len && rc == MPI_SUCCESS) {
                    sg.add(v, w.sub(r, me) + half, len * esz);
                    if (!fault_drop_flags(me, seq)) fl.push_back(w.flags(r) + me);
                }
            }
            const size_t mylen = o < mycnt ? std::min(qh_el, mycnt - o) : 0;
            if (rc == MPI_SUCCESS) {
                hipError_t e = launch_push_wait(sg.src.data(), sg.dst.data(), sg.n.data(), (int)sg.src.size(),
                                                fl.data(), (int)fl.size(), seq, counter + kCountWords,
                                                w.flags(me), mylen ? p : 0, me, err_dev, s);
                if (e != hipSuccess) rc = hip_fail(e, "reduce_scatter push");
            }
            if (rc == MPI_SUCCESS && mylen) {
                char* ro = out_window ? out : out + o * esz;
                rc = run_rank_tree(op.opidx, k, t, subs, esz, 0, mylen, ro, s);
                if (rc == MPI_SUCCESS && out_window) rc = copy_async(dst + o * esz, ro, mylen * esz, s);
            }
            if (rc == MPI_SUCCESS && ri + 2 < nrounds) {     // this round's half is read: free two rounds on
                hipError_t e = launch_post_flags(done_to.data(), (int)done_to.size(), seq, s);
                if (e != hipSuccess) rc = hip_fail(e, "reduce_scatter done flags");
            }
            tp->rd_parity ^= 1;
        }
        if (rc == MPI_SUCCESS && mycnt && in_place) rc = copy_async(dst, out, mycnt * esz, s);
        ++g_stats.flag_calls;
        const int rs = sync_stream(s, "reduce_scatter one-step");
        if (rc == MPI_SUCCESS) rc = rs;
        if (rc == MPI_SUCCESS && __atomic_load_n(err_host, __ATOMIC_ACQUIRE))
            rc = flag_timeout("reduce_scatter", me, __atomic_load_n(err_host, __ATOMIC_ACQUIRE), seq);
        tp->post_done(seq);
        tp->window_open = true;
        trace("reduce_scatter: done (GPU flags, %zu round(s), last seq %llu) rc=%d", nrounds, seq, rc);
        return rc;
    }
    // scratch: [hold: in-place results][stage: host-resident input pieces]
    const size_t hold_b = in_place ? ((mycnt * esz + 255) & ~(size_t)255) : 0;
    const size_t stage_b = bs.place == Place::Device ? 0 : (size_t)p * qe * esz;
    char* scratch = nullptr;
    if (hold_b + stage_b) {
        scratch = dev_scratch(hold_b + stage_b);
        if (!scratch) { set_error("reduce_scatter: scratch allocation failed"); return MPI_ERR_NO_MEM; }
    }
    char* hold = scratch;
    char* stage = scratch ? scratch + hold_b : nullptr;
    std::vector<char*> subs((size_t)p);
    for (int r = 0; r < p; ++r) subs[r] = w.sub(me, r);
    for (size_t o = 0; o < maxcnt && rc == MPI_SUCCESS; o += qe) {
        // my contribution to every destination's block range [o, o+qe)
        Segs scatter;
        for (int r = 0; r < p && rc == MPI_SUCCESS; ++r) {
            const size_t cnt = (size_t)recvcounts[r];
            if (o >= cnt) continue;
            const size_t len = std::min(qe, cnt - o);
            const char* v = nullptr;
            rc = device_view(bs, src, (disp[r] + o) * esz, len * esz, stage ? stage + (size_t)r * qe * esz : nullptr,
                             s, &v);
            if (r == me) subs[(size_t)me] = const_cast<char*>(v);   // read in place
            else scatter.add(v, w.sub(r, me), len * esz);
        }
        if (rc == MPI_SUCCESS) rc = scatter.run(s, "reduce_scatter scatter");
        if (rc == MPI_SUCCESS) rc = sync_stream(s, "reduce_scatter scatter");
        if (rc == MPI_SUCCESS) rc = tp->barrier();                                  // A
        if (rc != MPI_SUCCESS) break;
        if (o < mycnt) {
            const size_t len = std::min(qe, mycnt - o);
            // In place, recvbuf is still our input for later rounds: results go
            // to a private device scratch and are copied out at the end.
            char* out = in_place ? hold + o * esz
                                 : (bd.place == Place::Device ? static_cast<char*>(bd.dev) + o * esz : w.out(me));
            rc = run_rank_tree(op.opidx, k, t, subs, esz, 0, len, out, s);
            if (rc == MPI_SUCCESS && out == w.out(me)) rc = copy_async(dst + o * esz, out, len * esz, s);
            if (rc == MPI_SUCCESS) rc = sync_stream(s, "reduce_scatter reduce");
        }
        if (rc == MPI_SUCCESS) rc = tp->barrier();                                  // B
    }
    if (rc == MPI_SUCCESS && in_place && mycnt) {
        rc = copy_async(recvbuf, hold, mycnt * esz, s);
        if (rc == MPI_SUCCESS) rc = sync_stream(s, "reduce_scatter result");
    }
    trace("reduce_scatter: done rc=%d", rc);
    return rc;
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

// MPI_Reduce with a user function (host code): every contribution is gathered
// to host memory and the reference's binomial tree is evaluated with the
// user's function (reduce.cpp:440-540): relative ranks from lroot = root for
// commutative ops, else from 0 with the result sent to root; the parent
// combines a child's buffer as `in` (commutative) or as `inout` with its own
// as `in` (non-commutative, "the sender is above us").
int host_user_reduce(Comm* c, const void* sendbuf, void* recvbuf, size_t count, MPI_Datatype dt,
                     const OpRef& op, int root)
{
    const int p = c->size, me = c->rank;
    const Img m = img_of(dt, count);
    const size_t bytes = m.bytes;
    std::vector<char> mine(bytes), all((size_t)p * bytes);
    int rc = img_load(m, sendbuf == MPI_IN_PLACE ? recvbuf : sendbuf, mine.data());
    if (rc == MPI_SUCCESS) rc = c->tp->allgather(mine.data(), bytes, all.data());
    if (rc != MPI_SUCCESS || me != root) return rc;
    auto call = [&](const char* in, char* io) { img_call(op, dt, m, count, in - m.lo, io - m.lo); };
    const int lroot = op.commutative ? root : 0;
    auto buf = [&](int rel) { return all.data() + (size_t)((rel + lroot) % p) * bytes; };
    std::vector<char> tmp(bytes);
    for (int mask = 1; mask < p; mask <<= 1) {
        for (int rel = 0; rel < p; rel += 2 * mask) {     // receivers at this level
            const int src = rel | mask;
            if (src >= p) continue;
            if (op.commutative) {
                call(buf(src), buf(rel));
            } else {
                memcpy(tmp.data(), buf(src), bytes);
                call(buf(rel), tmp.data());
                memcpy(buf(rel), tmp.data(), bytes);
            }
        }
    }
    return img_store(m, count, buf(0) - m.lo, recvbuf);
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

namespace {

// MPI_Scan / MPI_Exscan: the reference builds a recursive-doubling task list
// (IscanBuildTaskList reduce.cpp:5285-5576, IexscanBuildTaskList :5671-5960,
// NbcTask::ExecuteScan tasks.cpp:694-766).  At step mask, rank r exchanges its
// partial result with dst = r ^ mask; if r > dst it folds the received value
// into both its partial and its result (Uop(tmp, partial), Uop(tmp, recvbuf);
// the first such step of Exscan copies tmp into recvbuf), else only into its
// partial.  The schedule is run step by step here, the exchange going through
// the IPC windows, so every combine has the reference's operands and roles.
int host_user_scan(Comm* c, const void* sendbuf, void* recvbuf, size_t count, MPI_Datatype dt,
                   const OpRef& op, bool exclusive)
{
    const int p = c->size, me = c->rank;
    const Img m = img_of(dt, count);
    const size_t bytes = m.bytes;
    std::vector<char> mine(bytes), all((size_t)p * bytes);
    int rc = img_load(m, sendbuf == MPI_IN_PLACE ? recvbuf : sendbuf, mine.data());
    if (rc == MPI_SUCCESS) rc = c->tp->allgather(mine.data(), bytes, all.data());
    if (rc != MPI_SUCCESS) return rc;
    auto call = [&](const char* in, char* io) { img_call(op, dt, m, count, in - m.lo, io - m.lo); };
    std::vector<std::vector<char>> part((size_t)p), res((size_t)p);
    std::vector<bool> have((size_t)p, !exclusive);
    for (int r = 0; r < p; ++r) {
        part[r].assign(all.begin() + (size_t)r * bytes, all.begin() + (size_t)(r + 1) * bytes);
        res[r] = part[r];
    }
    for (int mask = 1; mask < p; mask <<= 1) {
        std::vector<std::vector<char>> snap = part;
        const bool last = (mask << 1) >= p;
        for (int r = 0; r < p; ++r) {
            const int dst = r ^ mask;
            if (dst >= p || (last && r < dst)) continue;
            std::vector<char> tmp = snap[dst];
            if (r > dst) {
                call(tmp.data(), part[r].data());
                if (exclusive && !have[r]) { res[r] = tmp; have[r] = true; }
                else call(tmp.data(), res[r].data());
            } else if (op.commutative) {
                call(tmp.data(), part[r].data());
            } else {
                call(part[r].data(), tmp.data());
                part[r] = tmp;
            }
        }
    }
    if (exclusive && !have[me]) return MPI_SUCCESS;     // rank 0: recvbuf undefined
    return img_store(m, count, res[me].data() - m.lo, recvbuf);
}

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
    hipError_t e = launch_tree_spec(opidx, k, t, out, n, s);
    return e == hipSuccess ? MPI_SUCCESS : hip_fail(e, "scan combine");
}

int do_scan(Comm* c, const void* sendbuf, void* recvbuf, size_t count, MPI_Datatype dt,
            const OpRef& op, bool exclusive)
{
    if (op.dev_fn) return devop_scan(c, sendbuf, recvbuf, count, dt, op, exclusive);
    if (op.opidx == O_NULL) return host_user_scan(c, sendbuf, recvbuf, count, dt, op, exclusive);
    int rc = ensure_device();
    if (rc != MPI_SUCCESS) return rc;
    Transport* tp = c->tp;
    const int p = c->size, me = c->rank;
    const Kind k = type_info(dt)->kind;
    const size_t esz = (size_t)type_info(dt)->size, bytes = count * esz;
    hipStream_t s = tp->stream();
    const char* src = static_cast<const char*>(sendbuf == MPI_IN_PLACE ? recvbuf : sendbuf);
    // GPU-synchronised when the vector fits half an IN sub-slot (count, type,
    // p and the environment decide: the same on every rank)
    const size_t Qh = (sub_len(chunk_bytes(), p) / 2) & ~(size_t)255;
    const bool flags = p >= 2 && p <= 32 && tp->has_done() && bytes <= Qh && bytes <= two_step_max(tp);
    Windows w;
    if ((rc = get_windows(tp, &w, flags)) != MPI_SUCCESS) return rc;
    // Each step's partial is PUSHED into the consumer's IN window (an xGMI
    // remote write) and combined there from local HBM; two alternating halves
    // of IN: a peer writes step i+2's half only after the barrier of step i+1,
    // which this rank reaches after finishing its reads of step i.
    size_t ce = w.C / 2 / esz;
    ce -= ce % 16;
    if (ce == 0) { set_error("scan: window too small"); return MPI_ERR_INTERN; }
    const size_t bstride = (bytes + 255) & ~(size_t)255;
    char* partial = dev_scratch(4 * bstride + 256);
    if (!partial) { set_error("scan: scratch allocation failed"); return MPI_ERR_NO_MEM; }
    char* res = partial + bstride;
    char* src_stage = res + bstride;     // host operands the kernels cannot address
    char* dst_stage = src_stage + bstride;
    BufInfo bs = classify(src), bd = classify(recvbuf);
    PinHold pins;                        // host buffers: device aliases for the call
    pins.sync_before_release(s);
    alias_host_operands(pins, true, src, bytes, &bs, recvbuf, bytes, &bd);
    const char* srcv = bs.place == Place::Device ? static_cast<const char*>(bs.dev) : src;
    void* dstv = bd.place == Place::Device ? bd.dev : recvbuf;
    bool have = !exclusive;
    if (flags) {
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
        const size_t half = (size_t)tp->rd_parity * Qh;
        const unsigned long long seq = ++tp->rd_seq;
        int* err_host = nullptr;
        int* err_dev = wait_err_word(&err_host);
        unsigned* counter = tp->push_counter();
        if (!err_dev || !counter) { set_error("scan: flag word allocation failed"); return MPI_ERR_NO_MEM; }
        *err_host = 0;
        // the kernels read the send buffer and write recvbuf in place when
        // they are device memory (or pinned aliases); host memory is staged
        const bool src_dev = bs.place == Place::Device, dst_dev = bd.place == Place::Device;
        if (!src_dev) {
            rc = copy_async(src_stage, src, bytes, s);
            srcv = src_stage;
        }
        const char* cur_p = srcv;                       // current partial
        const char* cur_r = exclusive ? nullptr : srcv; // current result (have)
        bool same = !exclusive;                         // partial and result hold one value
        char* outv = dst_dev ? static_cast<char*>(dstv) : dst_stage;
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
                                            counter + kCountWords,
                                            use ? w.flags(me) + kScanFlags + dst : w.flags(me), use ? 1 : 0, -1,
                                            err_dev, s);
            if (e != hipSuccess) { rc = hip_fail(e, "scan push"); break; }
            if (!use) continue;
            const char* tmp = w.sub(me, dst) + half;
            // the partial is read again only by a later step's push or combine
            char* np = last ? nullptr : partial;
            if (me > dst) {
                char* nr = last ? outv : res;
                if (have && same) {                      // one combine, stored twice
                    rc = np ? combine2(op.opidx, k, cur_p, tmp, np, count, s, nr)
                            : combine2(op.opidx, k, cur_r, tmp, nr, count, s);
                } else {
                    if (np) rc = combine2(op.opidx, k, cur_p, tmp, np, count, s);
                    if (rc == MPI_SUCCESS)
                        rc = have ? combine2(op.opidx, k, cur_r, tmp, nr, count, s) : copy_async(nr, tmp, bytes, s);
                    same = false;
                }
                cur_p = np;
                cur_r = nr;
                have = true;
            } else {                                     // never the last step (use)
                rc = combine2(op.opidx, k, cur_p, tmp, partial, count, s);
                cur_p = partial;
                same = false;
            }
        }
        // a result that never left the send buffer or the scratch (rank 0 of an
        // inclusive scan, or a last step that did not fold) goes to recvbuf
        if (rc == MPI_SUCCESS && have && (cur_r != outv || !dst_dev))
            rc = copy_async(dst_dev ? static_cast<void*>(outv) : recvbuf, cur_r, bytes, s);
        const int rs = sync_stream(s, "scan");
        if (rc == MPI_SUCCESS) rc = rs;
        if (rc == MPI_SUCCESS && __atomic_load_n(err_host, __ATOMIC_ACQUIRE))
            rc = flag_timeout("scan", me, __atomic_load_n(err_host, __ATOMIC_ACQUIRE), seq, false);
        tp->post_done(seq);
        tp->rd_parity ^= 1;
        tp->window_open = true;
        return rc;
    }
    rc = copy_async(partial, srcv, bytes, s);
    if (rc == MPI_SUCCESS && !exclusive) rc = copy_async(res, srcv, bytes, s);
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
                char* stage = w.in(dst) + (size_t)slot * (w.C / 2);
                rc = copy_async(stage, partial + o * esz, len * esz, s);   // partial at step start
                if (rc == MPI_SUCCESS) rc = sync_stream(s, "scan push");
            }
            if (rc == MPI_SUCCESS) rc = tp->barrier();
            if (rc != MPI_SUCCESS || !use) continue;
            const char* tmp = w.in(me) + (size_t)slot * (w.C / 2);
            char* pp = partial + o * esz;
            char* rr = res + o * esz;
            if (me > dst) {
                rc = combine2(op.opidx, k, pp, tmp, pp, len, s);
                if (rc == MPI_SUCCESS)
                    rc = have ? combine2(op.opidx, k, rr, tmp, rr, len, s) : copy_async(rr, tmp, len * esz, s);
            } else {
                rc = combine2(op.opidx, k, pp, tmp, pp, len, s);             // builtins commute
            }
            if (rc == MPI_SUCCESS) rc = sync_stream(s, "scan step");
        }
        if (use && me > dst) have = true;
    }
    if (rc == MPI_SUCCESS) rc = tp->barrier();
    if (rc == MPI_SUCCESS && have) {
        rc = copy_async(dstv, res, bytes, s);
        if (rc == MPI_SUCCESS) rc = sync_stream(s, "scan result");
    }
    return rc;
}

}  // namespace

int engine_scan(Comm* c, const void* sendbuf, void* recvbuf, size_t count, MPI_Datatype dt,
                const OpRef& op, bool exclusive)
{
    return worker().run([=] { return do_scan(c, sendbuf, recvbuf, count, dt, op, exclusive); });
}

}  // namespace msx
