// msx_devop.cpp — the reduction collectives with a device-resident user op
// (msx_op_create_device).  Each executes the combine plan the host user-op
// path executes (userop_plan, msx_schedule.cpp; tests/test_userop_plan_cpu.py
// pins it to the reference's order) -- but the contributions stay in HBM:
//
//   gather   : a device gather over the engine windows, chunked by the
//              sub-slot length under host barriers (the schedule of
//              do_allreduce's host-barrier loop); a rank receives only what it
//              will combine
//   evaluate : the user's function on tp->stream() over blocks of the engine's
//              device scratch, one stream sync before the result is stored
//
// The plan is the value of ONE rank, every gathered block an operand exactly
// once, so the combines run in place on the gathered blocks: p - 1 calls for
// allreduce, reduce (root only) and commutative reduce_scatter (over the
// rank's block), at most p - 1 for scan / exscan.  Non-commutative
// reduce_scatter is an allreduce of the whole vector.
//
// An op with a tree function (msx_op_create_device_tree) evaluates the same
// value in ONE call: devop_tree_spec (msx_schedule.cpp) names the plan's tree,
// the sources are the gathered blocks and the result lands in the block of the
// rank's own contribution.  Scan / exscan (partials that are not one such
// tree), shapes beyond 16 leaves and a declined call run the plan.
#include "msx_engine.h"

#include <algorithm>

namespace msx {

namespace {

// one image block of the engine's device scratch: whole 256-byte lines
size_t block_stride(size_t bytes) { return (std::max(bytes, (size_t)1) + 255) & ~(size_t)255; }

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

// What the four collectives share.  A call opens (device, stream, windows),
// takes its blocks, gathers, evaluates; an entry point states only what it
// gathers, which plan it uses and which part of the result it stores.
struct DevCall {
    Comm* c;
    const OpRef& op;
    MPI_Datatype dt;
    Img m;                    // the image of the `count` elements the op combines
    size_t count;
    hipStream_t s = nullptr;
    Windows w;
    std::vector<char*> x;     // x[r]: the block of rank r's contribution
    int rc;

    DevCall(Comm* c_, const OpRef& op_, MPI_Datatype dt_, size_t count_)
        : c(c_), op(op_), dt(dt_), m(img_of(dt_, count_)), count(count_), rc(ensure_device())
    {
        if (rc != MPI_SUCCESS) return;
        s = c->tp->stream();
        rc = get_windows(c->tp, &w);
    }

    // x[0..n-1] <- n image blocks of the engine's device scratch; -> the
    // `extra` bytes behind them, nullptr (and rc) when there is no memory
    char* blocks(int n, size_t extra = 0)
    {
        const size_t stride = block_stride(m.bytes);
        char* base = dev_scratch((size_t)n * stride + extra);
        if (!base) {
            set_error("device user op: scratch allocation failed");
            rc = MPI_ERR_NO_MEM;
            return nullptr;
        }
        x.assign((size_t)c->size, nullptr);
        for (int r = 0; r < n; ++r) x[(size_t)r] = base + (size_t)r * stride;
        return base + (size_t)n * stride;
    }

    // dev_gather into x; a rank that failed so far still passes the gather's barriers
    void gather(const std::vector<const char*>& send, const std::vector<size_t>& send_n,
                const std::vector<size_t>& recv_n, size_t max_n)
    {
        const int rg = dev_gather(c->tp, w, send, send_n, x, recv_n, max_n, s);
        if (rc == MPI_SUCCESS) rc = rg;
    }
    // every contribution to every rank (allreduce, scan): x[me] <- the image
    // of `buf`, x[r] <- rank r's
    void gather_all(const void* buf)
    {
        const size_t p = (size_t)c->size;
        char* mine = x[(size_t)c->rank];
        rc = img_load(m, buf, mine);
        const std::vector<size_t> n(p, m.bytes);
        gather(std::vector<const char*>(p, mine), n, n, m.bytes);
    }

    // io = in (op) io over image starts (typed bases = start - lo); enqueue only
    void call(const char* in, char* io)
    {
        if (rc == MPI_SUCCESS) rc = device_op_call(op, dt, in - m.lo, io - m.lo, count, s);
    }
    // The whole evaluation as one call of the op's tree function:
    // devop_tree_spec's tree over the blocks, the result into `out`.  false:
    // nothing was enqueued (no tree function, no such tree, a decline) and
    // the plan's pairwise calls are due.
    bool tree(UserColl which, int n, size_t gate_count, char* out)
    {
        if (!op.dev_tree) return false;
        RankTree t;
        int in_left = 0;
        if (!devop_tree_spec(which, c->size, n, op.commutative, gate_count, gate_type_size(dt, false), &t, &in_left))
            return false;
        const void* srcs[32];
        for (int i = 0; i < 32; ++i) srcs[i] = t.src[i] >= 0 ? x[(size_t)t.src[i]] - m.lo : nullptr;
        const int r = device_op_tree_call(op, dt, srcs, t.P, t.pairmask, t.nleaves, t.chain ? 1 : 0, in_left,
                                          out - m.lo, count, s);
        if (r == MSX_TREE_DECLINED) return false;
        rc = r;
        return true;
    }

    // The value of collective `which` for rank (or root) n over the gathered
    // blocks -- the tree function first, into the block of the rank's own
    // contribution, else the plan -- then one sync, and out_count elements
    // from typed byte `off` of the value through the datatype into recvbuf
    // (MPIR_Localcopy: only the mapped bytes of a derived recvbuf are written).
    int evaluate(UserColl which, int n, bool exclusive, size_t gate_count, void* recvbuf, int64_t off,
                 size_t out_count)
    {
        if (rc != MPI_SUCCESS) return rc;
        char* res = x[(size_t)c->rank];
        if (!tree(which, n, gate_count, res)) {
            const CombinePlan plan =
                userop_plan(which, c->size, n, op.commutative, exclusive, gate_count, gate_type_size(dt, false));
            for (const CombineStep& st : plan.steps) call(x[(size_t)st.in], x[(size_t)st.io]);
            res = plan.result < 0 ? nullptr : x[(size_t)plan.result];
        }
        const int rs = sync_stream(s, "device op evaluate");
        if (rc != MPI_SUCCESS) return rc;
        if (rs != MPI_SUCCESS) return rs;
        if (!res || out_count == 0) return MPI_SUCCESS;          // exscan rank 0: recvbuf undefined
        return local_copy(res - m.lo + off, recvbuf, out_count, dt);
    }
};

}  // namespace

int devop_allreduce(Comm* c, const void* sendbuf, void* recvbuf, size_t count, MPI_Datatype dt, const OpRef& op)
{
    DevCall d(c, op, dt, count);
    if (d.rc != MPI_SUCCESS || !d.blocks(c->size)) return d.rc;
    d.gather_all(sendbuf == MPI_IN_PLACE ? recvbuf : sendbuf);
    return d.evaluate(UserColl::allreduce, c->rank, false, count, recvbuf, 0, count);
}

int devop_reduce(Comm* c, const void* sendbuf, void* recvbuf, size_t count, MPI_Datatype dt, const OpRef& op,
                 int root)
{
    const size_t p = (size_t)c->size;
    const int me = c->rank;
    DevCall d(c, op, dt, count);
    if (d.rc != MPI_SUCCESS || !d.blocks(me == root ? c->size : 1)) return d.rc;
    char* mine = d.x[(size_t)(me == root ? me : 0)];
    d.rc = img_load(d.m, sendbuf == MPI_IN_PLACE ? recvbuf : sendbuf, mine);
    // only the root combines: every other rank sends to it and receives nothing
    std::vector<size_t> send_n(p, 0), recv_n(p, 0);
    if (me == root) recv_n.assign(p, d.m.bytes);
    else send_n[(size_t)root] = d.m.bytes;
    d.gather(std::vector<const char*>(p, mine), send_n, recv_n, d.m.bytes);
    if (me != root) return d.rc;
    return d.evaluate(UserColl::reduce, root, false, count, recvbuf, 0, count);
}

int devop_reduce_scatter(Comm* c, const void* sendbuf, void* recvbuf, const int* recvcounts, MPI_Datatype dt,
                         const OpRef& op)
{
    const int p = c->size, me = c->rank;
    std::vector<size_t> disp((size_t)p + 1, 0);
    for (int r = 0; r < p; ++r) disp[(size_t)r + 1] = disp[(size_t)r] + (size_t)recvcounts[r];
    const size_t total = disp[(size_t)p], mycnt = (size_t)recvcounts[me];
    if (total == 0) return ensure_device();
    const void* src = sendbuf == MPI_IN_PLACE ? recvbuf : sendbuf;
    const Img mf = img_of(dt, total);
    const int64_t unit = mf.t ? mf.t->extent : (int64_t)mf.esz;

    if (!op.commutative) {
        // recursive doubling over the whole vector (MPIR_Reduce_scatter_non_commutative),
        // then block `me` of the result
        DevCall d(c, op, dt, total);
        if (d.rc != MPI_SUCCESS || !d.blocks(p)) return d.rc;
        d.gather_all(src);
        return d.evaluate(UserColl::reduce_scatter, me, false, total, recvbuf, (int64_t)disp[(size_t)me] * unit,
                          mycnt);
    }

    // commutative: each rank combines its own block only.  imgs[r] = the image
    // of block r, recvcounts[r] elements from typed offset disp[r] * unit.
    DevCall d(c, op, dt, mycnt);
    if (d.rc != MPI_SUCCESS) return d.rc;
    std::vector<Img> imgs((size_t)p);
    size_t max_n = 0;
    for (int r = 0; r < p; ++r) {
        imgs[(size_t)r] = img_of(dt, (size_t)recvcounts[r]);
        max_n = std::max(max_n, imgs[(size_t)r].bytes);
    }
    // blocks 0..p-1: every rank's contribution to my block; then, for a host
    // send buffer, the whole input staged once
    const bool src_dev = classify(static_cast<const char*>(src) + mf.lo).place == Place::Device;
    char* full = d.blocks(p, src_dev ? 0 : block_stride(mf.bytes));
    if (!full) return d.rc;
    const char* typed = static_cast<const char*>(src);      // typed base of the whole input, device memory
    if (!src_dev) {
        d.rc = img_load(mf, src, full);
        typed = full - mf.lo;
    }
    std::vector<const char*> send((size_t)p);
    std::vector<size_t> send_n((size_t)p), recv_n((size_t)p, d.m.bytes);
    for (int r = 0; r < p; ++r) {
        send[(size_t)r] = typed + (int64_t)disp[(size_t)r] * unit + imgs[(size_t)r].lo;
        send_n[(size_t)r] = imgs[(size_t)r].bytes;
    }
    if (d.rc == MPI_SUCCESS) d.rc = copy_async(d.x[(size_t)me], send[(size_t)me], d.m.bytes, d.s);   // my own piece
    d.gather(send, send_n, recv_n, max_n);
    if (mycnt == 0) return d.rc;
    return d.evaluate(UserColl::reduce_scatter, me, false, total, recvbuf, 0, mycnt);
}

int devop_scan(Comm* c, const void* sendbuf, void* recvbuf, size_t count, MPI_Datatype dt, const OpRef& op,
               bool exclusive)
{
    DevCall d(c, op, dt, count);
    if (d.rc != MPI_SUCCESS || !d.blocks(c->size)) return d.rc;
    d.gather_all(sendbuf == MPI_IN_PLACE ? recvbuf : sendbuf);
    return d.evaluate(UserColl::scan, c->rank, exclusive, count, recvbuf, 0, count);
}

}  // namespace msx
