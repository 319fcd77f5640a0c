// msx_devop.cpp — the reduction collectives with a device-resident user op
// (msx_op_create_device).  Each produces exactly the association and operand
// roles of the host user-op path (host_user_allreduce / _reduce / _scan and the
// user-op branch of do_reduce_scatter), which tests/test_collectives_cpu.py
// pins to the reference's order -- but the contributions stay in HBM:
//
//   gather   : a device gather over the engine windows, chunked by the
//              sub-slot length under host barriers (the schedule of
//              do_allreduce's host-barrier loop); a rank receives only what it
//              will combine
//   evaluate : the user's function on tp->stream() over blocks of the engine's
//              device scratch, one stream sync before the result is stored
//
// One rank evaluates only its OWN result.  The host path simulates every
// rank's schedule (O(p log p) combines); here the value of rank `me` is
// written as the expression tree the schedule builds for it, and every
// gathered block is a leaf of that tree exactly once, so the combines run in
// place on the gathered blocks: p - 1 calls for allreduce, reduce (root only)
// and commutative reduce_scatter (over the rank's block), at most p - 1 for
// scan / exscan.  Non-commutative reduce_scatter is an allreduce of the whole
// vector, as on the host path.
//
// An op with a tree function (msx_op_create_device_tree) evaluates the same
// value in ONE call: devop_tree_spec (msx_schedule.cpp) names the tree the
// calls above build, the sources are the gathered blocks and the result lands
// in the block of the rank's own contribution.  Scan / exscan (partials that
// are not one such tree), shapes beyond 16 leaves and a declined call keep the
// pairwise calls.
#include "msx_engine.h"

#include <algorithm>

namespace msx {

namespace {

// p image blocks of the engine's device scratch, `stride` bytes apart.
struct Blocks {
    char* base = nullptr;
    size_t stride = 0;
    char* at(int i) const { return base + (size_t)i * stride; }
};

size_t block_stride(size_t bytes) { return (std::max(bytes, (size_t)1) + 255) & ~(size_t)255; }

int blocks_get(int n, size_t bytes, Blocks* b)
{
    b->stride = block_stride(bytes);
    b->base = dev_scratch((size_t)n * b->stride);
    if (!b->base) { set_error("device user op: scratch allocation failed"); return MPI_ERR_NO_MEM; }
    return MPI_SUCCESS;
}

// The device gather.  send[r] / send_n[r]: the bytes this rank contributes to
// rank r (device memory; nothing when send_n[r] == 0); recv[r] / recv_n[r]:
// where rank r's contribution lands (recv_n[r] == send_n[me] on rank r).
// max_n: the longest piece any rank sends, the same on every rank, so all
// ranks pass the same barriers.  Per chunk of one sub-slot: my pieces into
// w.sub(r, me), barrier A, out of my own sub-slots, barrier B (a peer writes
// the next chunk into my window only after B).
int dev_gather(Transport* tp, const Windows& w, const std::vector<const char*>& send,
               const std::vector<size_t>& send_n, const std::vector<char*>& recv, const std::vector<size_t>& recv_n,
               size_t max_n, hipStream_t s)
{
    const int p = tp->size, me = tp->rank;
    if (w.Q == 0) { set_error("device user op: window too small"); return MPI_ERR_INTERN; }
    int rc = MPI_SUCCESS;
    for (size_t o = 0; o < max_n && rc == MPI_SUCCESS; o += w.Q) {
        Segs push;
        for (int r = 0; r < p; ++r)
            if (r != me && o < send_n[(size_t)r])
                push.add(send[(size_t)r] + o, w.sub(r, me), std::min(w.Q, send_n[(size_t)r] - o));
        rc = push.run(s, "device op gather push");
        if (rc == MPI_SUCCESS) rc = sync_stream(s, "device op gather push");
        if (rc == MPI_SUCCESS) rc = tp->barrier();                                  // A
        if (rc != MPI_SUCCESS) break;
        Segs pull;
        for (int r = 0; r < p; ++r)
            if (r != me && o < recv_n[(size_t)r])
                pull.add(w.sub(me, r), recv[(size_t)r] + o, std::min(w.Q, recv_n[(size_t)r] - o));
        rc = pull.run(s, "device op gather collect");
        if (rc == MPI_SUCCESS) rc = sync_stream(s, "device op gather collect");
        if (rc == MPI_SUCCESS) rc = tp->barrier();                                  // B
    }
    return rc;
}

// Everything one call shares: the op, the image of `count` elements, the stream.
struct Eval {
    const OpRef& op;
    MPI_Datatype dt;
    Img m;
    size_t count;
    hipStream_t s;
    int rc = MPI_SUCCESS;
    // io = in (op) io over image starts (typed bases = start - lo); enqueue only
    void call(const char* in, char* io)
    {
        if (rc == MPI_SUCCESS) rc = device_op_call(op, dt, in - m.lo, io - m.lo, count, s);
    }
    // The whole evaluation as one call of the op's tree function: collective
    // `which` of devop_tree_spec for rank (or root) n over the blocks x[r],
    // the result into `out`.  false: nothing was enqueued (no tree function, a
    // shape beyond 16 leaves or a decline) and the pairwise calls are due.
    bool tree(int which, int p, int n, size_t gate_count, const std::vector<char*>& x, char* out)
    {
        if (!op.dev_tree || rc != MPI_SUCCESS) return false;
        RankTree t;
        int in_left = 0;
        if (!devop_tree_spec(which, p, n, op.commutative, gate_count, gate_type_size(dt, false), &t, &in_left))
            return false;
        const void* srcs[32];
        for (int i = 0; i < 32; ++i) srcs[i] = t.src[i] >= 0 ? x[(size_t)t.src[i]] - m.lo : nullptr;
        const int r = device_op_tree_call(op, dt, srcs, t.P, t.pairmask, t.nleaves, t.chain ? 1 : 0, in_left,
                                          out - m.lo, count, s);
        if (r == MSX_TREE_DECLINED) return false;
        rc = r;
        return true;
    }
};

// The value recursive doubling leaves at newrank n after `level` steps
// (reduce.cpp:3890-3925 as host_user_allreduce runs it): the block that holds
// it.  x[r] = rank r's image, combined in place.
char* rd_value(Eval& ev, const std::vector<char*>& x, int p, bool commutative, int n, int level)
{
    const int rem = p - pof2_floor(p);
    const int r = real_of_newrank(n, p);
    if (level == 0) {
        if (r < 2 * rem) ev.call(x[(size_t)r - 1], x[(size_t)r]);     // the even neighbour folds into the odd rank
        return x[(size_t)r];
    }
    const int mask = 1 << (level - 1);
    const int dst = real_of_newrank(n ^ mask, p);
    char* a = rd_value(ev, x, p, commutative, n, level - 1);
    char* b = rd_value(ev, x, p, commutative, n ^ mask, level - 1);
    if (commutative || dst < r) {
        ev.call(b, a);
        return a;
    }
    ev.call(a, b);              // the partner's copy takes the result ("the sender is above us")
    return b;
}

char* eval_allreduce(Eval& ev, const std::vector<char*>& x, int p, int me, bool commutative)
{
    const int pof2 = pof2_floor(p), rem = p - pof2;
    const int src = (me < 2 * rem && (me & 1) == 0) ? me + 1 : me;   // a folded rank gets its odd neighbour's value
    int levels = 0;
    while ((1 << levels) < pof2) ++levels;
    return rd_value(ev, x, p, commutative, newrank_of(src, p), levels);
}

// host_user_reduce's binomial tree at the root (reduce.cpp:440-540)
char* eval_reduce(Eval& ev, std::vector<char*> x, int p, int root, bool commutative)
{
    const int lroot = commutative ? root : 0;
    auto buf = [&](int rel) -> char*& { return x[(size_t)((rel + lroot) % p)]; };
    for (int mask = 1; mask < p; mask <<= 1)
        for (int rel = 0; rel < p; rel += 2 * mask) {
            const int src = rel | mask;
            if (src >= p) continue;
            if (commutative) {
                ev.call(buf(src), buf(rel));
            } else {
                ev.call(buf(rel), buf(src));
                std::swap(buf(rel), buf(src));
            }
        }
    return buf(0);
}

// eval_tree_host over device blocks: x[r] = image of rank r's contribution
char* eval_tree_dev(Eval& ev, const RankTree& t, const std::vector<char*>& x)
{
    if (t.chain) {
        char* out = x[(size_t)t.src[0]];
        for (int k = 1; k < t.P; ++k) ev.call(x[(size_t)t.src[k]], out);
        return out;
    }
    const int nl = t.nleaves ? t.nleaves : t.P;
    std::vector<char*> v((size_t)nl);
    for (int k = 0; k < nl; ++k) {
        v[(size_t)k] = x[(size_t)t.src[2 * k]];
        if ((t.pairmask >> k) & 1u) ev.call(x[(size_t)t.src[2 * k + 1]], v[(size_t)k]);
    }
    for (int w = 1; w < t.P; w *= 2)
        for (int k = 0; k + w < t.P; k += 2 * w)
            if (k + w < nl) ev.call(v[(size_t)(k + w)], v[(size_t)k]);
    return v[0];
}

// rank r's partial after `steps` steps of host_user_scan's recursive doubling
char* scan_partial(Eval& ev, const std::vector<char*>& x, int p, bool commutative, int r, int steps)
{
    if (steps == 0) return x[(size_t)r];
    const int mask = 1 << (steps - 1);
    const bool last = (mask << 1) >= p;
    const int dst = r ^ mask;
    char* a = scan_partial(ev, x, p, commutative, r, steps - 1);
    if (dst >= p || (last && r < dst)) return a;
    char* b = scan_partial(ev, x, p, commutative, dst, steps - 1);
    if (r > dst || commutative) {
        ev.call(b, a);
        return a;
    }
    ev.call(a, b);
    return b;
}

// the result of rank me, or nullptr when it has none (rank 0 of an exscan)
char* eval_scan(Eval& ev, const std::vector<char*>& x, int p, int me, bool commutative, bool exclusive)
{
    char* res = exclusive ? nullptr : x[(size_t)me];
    int step = 0;
    for (int mask = 1; mask < p; mask <<= 1, ++step) {
        const int dst = me ^ mask;
        const bool last = (mask << 1) >= p;
        if (dst >= p || (last && me < dst) || me < dst) continue;
        char* tmp = scan_partial(ev, x, p, commutative, dst, step);
        if (!res) res = tmp;
        else ev.call(tmp, res);
    }
    return res;
}

// evaluation done: one sync, then the result through the datatype into recvbuf
// (MPIR_Localcopy: only the mapped bytes of a derived recvbuf are written)
int finish(Eval& ev, const char* res_typed_base, void* recvbuf, size_t count)
{
    const int rs = sync_stream(ev.s, "device op evaluate");
    if (ev.rc != MPI_SUCCESS) return ev.rc;
    if (rs != MPI_SUCCESS) return rs;
    if (!res_typed_base || count == 0) return MPI_SUCCESS;
    return local_copy(res_typed_base, recvbuf, count, ev.dt);
}

// every contribution to every rank (allreduce, scan): x[r] <- rank r's image
int gather_all(Comm* c, const Windows& w, const Blocks& b, size_t bytes, std::vector<char*>* x, hipStream_t s)
{
    const int p = c->size, me = c->rank;
    std::vector<const char*> send((size_t)p, b.at(me));
    std::vector<size_t> n((size_t)p, bytes);
    x->resize((size_t)p);
    for (int r = 0; r < p; ++r) (*x)[(size_t)r] = b.at(r);
    return dev_gather(c->tp, w, send, n, *x, n, bytes, s);
}

}  // namespace

int devop_allreduce(Comm* c, const void* sendbuf, void* recvbuf, size_t count, MPI_Datatype dt, const OpRef& op)
{
    int rc = ensure_device();
    if (rc != MPI_SUCCESS) return rc;
    const int p = c->size, me = c->rank;
    Eval ev{op, dt, img_of(dt, count), count, c->tp->stream()};
    Windows w;
    if ((rc = get_windows(c->tp, &w)) != MPI_SUCCESS) return rc;
    Blocks b;
    if ((rc = blocks_get(p, ev.m.bytes, &b)) != MPI_SUCCESS) return rc;
    rc = img_load(ev.m, sendbuf == MPI_IN_PLACE ? recvbuf : sendbuf, b.at(me));
    // a rank that failed so far still passes the gather's barriers
    std::vector<char*> x;
    const int rg = gather_all(c, w, b, ev.m.bytes, &x, ev.s);
    if (rc == MPI_SUCCESS) rc = rg;
    if (rc != MPI_SUCCESS) return rc;
    char* res = ev.tree(0, p, me, count, x, x[(size_t)me]) ? x[(size_t)me] : eval_allreduce(ev, x, p, me, op.commutative);
    return finish(ev, res - ev.m.lo, recvbuf, count);
}

int devop_reduce(Comm* c, const void* sendbuf, void* recvbuf, size_t count, MPI_Datatype dt, const OpRef& op,
                 int root)
{
    int rc = ensure_device();
    if (rc != MPI_SUCCESS) return rc;
    const int p = c->size, me = c->rank;
    Eval ev{op, dt, img_of(dt, count), count, c->tp->stream()};
    Windows w;
    if ((rc = get_windows(c->tp, &w)) != MPI_SUCCESS) return rc;
    Blocks b;
    if ((rc = blocks_get(me == root ? p : 1, ev.m.bytes, &b)) != MPI_SUCCESS) return rc;
    char* mine = me == root ? b.at(me) : b.at(0);
    rc = img_load(ev.m, sendbuf == MPI_IN_PLACE ? recvbuf : sendbuf, mine);
    // only the root combines: every other rank sends to it and receives nothing
    std::vector<const char*> send((size_t)p, mine);
    std::vector<size_t> send_n((size_t)p, 0), recv_n((size_t)p, 0);
    std::vector<char*> x((size_t)p, nullptr);
    if (me == root) {
        for (int r = 0; r < p; ++r) {
            x[(size_t)r] = b.at(r);
            recv_n[(size_t)r] = ev.m.bytes;
        }
    } else {
        send_n[(size_t)root] = ev.m.bytes;
    }
    const int rg = dev_gather(c->tp, w, send, send_n, x, recv_n, ev.m.bytes, ev.s);
    if (rc == MPI_SUCCESS) rc = rg;
    if (rc != MPI_SUCCESS || me != root) return rc;
    char* res = ev.tree(1, p, root, count, x, x[(size_t)me]) ? x[(size_t)me] : eval_reduce(ev, x, p, root, op.commutative);
    return finish(ev, res - ev.m.lo, recvbuf, count);
}

int devop_reduce_scatter(Comm* c, const void* sendbuf, void* recvbuf, const int* recvcounts, MPI_Datatype dt,
                         const OpRef& op)
{
    int rc = ensure_device();
    if (rc != MPI_SUCCESS) return rc;
    const int p = c->size, me = c->rank;
    std::vector<size_t> disp((size_t)p + 1, 0);
    for (int r = 0; r < p; ++r) disp[(size_t)r + 1] = disp[(size_t)r] + (size_t)recvcounts[r];
    const size_t total = disp[(size_t)p], mycnt = (size_t)recvcounts[me];
    if (total == 0) return MPI_SUCCESS;
    const void* src = sendbuf == MPI_IN_PLACE ? recvbuf : sendbuf;
    const Img mf = img_of(dt, total);
    const int64_t unit = mf.t ? mf.t->extent : (int64_t)mf.esz;
    hipStream_t s = c->tp->stream();
    Windows w;
    if ((rc = get_windows(c->tp, &w)) != MPI_SUCCESS) return rc;

    if (!op.commutative) {
        // recursive doubling over the whole vector (MPIR_Reduce_scatter_non_commutative),
        // then block `me` of the result
        Eval ev{op, dt, mf, total, s};
        Blocks b;
        if ((rc = blocks_get(p, mf.bytes, &b)) != MPI_SUCCESS) return rc;
        rc = img_load(mf, src, b.at(me));
        std::vector<char*> x;
        const int rg = gather_all(c, w, b, mf.bytes, &x, s);
        if (rc == MPI_SUCCESS) rc = rg;
        if (rc != MPI_SUCCESS) return rc;
        char* res = ev.tree(2, p, me, total, x, x[(size_t)me]) ? x[(size_t)me] : eval_allreduce(ev, x, p, me, false);
        return finish(ev, res - mf.lo + (int64_t)disp[(size_t)me] * unit, recvbuf, mycnt);
    }

    // commutative: each rank combines its own block only.  imgs[r] = the image
    // of block r, recvcounts[r] elements from typed offset disp[r] * unit.
    std::vector<Img> imgs((size_t)p);
    size_t max_n = 0;
    for (int r = 0; r < p; ++r) {
        imgs[(size_t)r] = img_of(dt, (size_t)recvcounts[r]);
        max_n = std::max(max_n, imgs[(size_t)r].bytes);
    }
    const Img& mb = imgs[(size_t)me];
    Eval ev{op, dt, mb, mycnt, s};
    // blocks 0..p-1: every rank's contribution to my block; then, for a host
    // send buffer, the whole input staged once
    const bool src_dev = classify(static_cast<const char*>(src) + mf.lo).place == Place::Device;
    const size_t bs = block_stride(mb.bytes);
    char* scratch = dev_scratch((size_t)p * bs + (src_dev ? 0 : block_stride(mf.bytes)));
    if (!scratch) { set_error("device user op: scratch allocation failed"); return MPI_ERR_NO_MEM; }
    Blocks b{scratch, bs};
    const char* typed = static_cast<const char*>(src);      // typed base of the whole input, device memory
    if (!src_dev) {
        char* full = scratch + (size_t)p * bs;
        rc = img_load(mf, src, full);
        typed = full - mf.lo;
    }
    std::vector<const char*> send((size_t)p);
    std::vector<size_t> send_n((size_t)p), recv_n((size_t)p, mb.bytes);
    std::vector<char*> x((size_t)p);
    for (int r = 0; r < p; ++r) {
        send[(size_t)r] = typed + (int64_t)disp[(size_t)r] * unit + imgs[(size_t)r].lo;
        send_n[(size_t)r] = imgs[(size_t)r].bytes;
        x[(size_t)r] = b.at(r);
    }
    if (rc == MPI_SUCCESS) rc = copy_async(b.at(me), send[(size_t)me], mb.bytes, s);   // my own piece
    const int rg = dev_gather(c->tp, w, send, send_n, x, recv_n, max_n, s);
    if (rc == MPI_SUCCESS) rc = rg;
    if (rc != MPI_SUCCESS || mycnt == 0) return rc;
    const int algo = reduce_scatter_algo(p, total, gate_type_size(dt, false), true);
    const int n = newrank_of(me, p);
    const RankTree t = (algo == A_RS_PAIRWISE) ? tree_pairwise(p, me)
                                               : tree_reduce_scatter(p, n >= 0 ? n : newrank_of(me + 1, p));
    char* res = ev.tree(2, p, me, total, x, x[(size_t)me]) ? x[(size_t)me] : eval_tree_dev(ev, t, x);
    return finish(ev, res - mb.lo, recvbuf, mycnt);
}

int devop_scan(Comm* c, const void* sendbuf, void* recvbuf, size_t count, MPI_Datatype dt, const OpRef& op,
               bool exclusive)
{
    int rc = ensure_device();
    if (rc != MPI_SUCCESS) return rc;
    const int p = c->size, me = c->rank;
    Eval ev{op, dt, img_of(dt, count), count, c->tp->stream()};
    Windows w;
    if ((rc = get_windows(c->tp, &w)) != MPI_SUCCESS) return rc;
    Blocks b;
    if ((rc = blocks_get(p, ev.m.bytes, &b)) != MPI_SUCCESS) return rc;
    rc = img_load(ev.m, sendbuf == MPI_IN_PLACE ? recvbuf : sendbuf, b.at(me));
    std::vector<char*> x;
    const int rg = gather_all(c, w, b, ev.m.bytes, &x, ev.s);
    if (rc == MPI_SUCCESS) rc = rg;
    if (rc != MPI_SUCCESS) return rc;
    char* res = eval_scan(ev, x, p, me, op.commutative, exclusive);
    return finish(ev, res ? res - ev.m.lo : nullptr, recvbuf, count);   // exscan rank 0: recvbuf undefined
}

}  // namespace msx
