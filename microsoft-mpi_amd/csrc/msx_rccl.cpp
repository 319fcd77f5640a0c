// msx_rccl.cpp — the RCCL loader and both RCCL planes (send/recv trees in
// reference order, and RCCL's own collectives).  The only file that includes
// <rccl/rccl.h>; the per-transport communicator maps are private to it.
#include "msx_engine.h"

#include <dlfcn.h>
#include <algorithm>
#include <map>
#include <stdlib.h>
#include <string.h>

#include <rccl/rccl.h>

namespace msx {

// ---- RCCL plane (MSX_TRANSPORT=rccl) -------------------------------------------
// The same reference-order trees, with the bytes moved by RCCL point-to-point
// (ncclSend/ncclRecv groups over xGMI) instead of IPC windows: no host
// barriers, no peer mappings, user device buffers sent and received in place,
// everything ordered on the engine stream.  RCCL needs one GPU per rank; a
// communicator whose ranks share a GPU keeps the IPC window engine.
// librccl is opened lazily so the library has no link-time RCCL dependency.
namespace {
struct RcclApi {
    decltype(&ncclGetUniqueId) get_id = nullptr;
    decltype(&ncclCommInitRank) init_rank = nullptr;
    decltype(&ncclCommDestroy) destroy = nullptr;
    decltype(&ncclSend) send = nullptr;
    decltype(&ncclRecv) recv = nullptr;
    decltype(&ncclGroupStart) group_start = nullptr;
    decltype(&ncclGroupEnd) group_end = nullptr;
    decltype(&ncclGetErrorString) err = nullptr;
    // RCCL's own collectives (MSX_TRANSPORT=rccl_native)
    decltype(&ncclAllReduce) all_reduce = nullptr;
    decltype(&ncclReduce) reduce = nullptr;
    decltype(&ncclReduceScatter) reduce_scatter = nullptr;
    bool ok = false;
};

const RcclApi* rccl_api()
{
    static RcclApi a = [] {
        RcclApi r;
        void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
        if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
        if (!h) return r;
        r.get_id = reinterpret_cast<decltype(r.get_id)>(dlsym(h, "ncclGetUniqueId"));
        r.init_rank = reinterpret_cast<decltype(r.init_rank)>(dlsym(h, "ncclCommInitRank"));
        r.destroy = reinterpret_cast<decltype(r.destroy)>(dlsym(h, "ncclCommDestroy"));
        r.send = reinterpret_cast<decltype(r.send)>(dlsym(h, "ncclSend"));
        r.recv = reinterpret_cast<decltype(r.recv)>(dlsym(h, "ncclRecv"));
        r.group_start = reinterpret_cast<decltype(r.group_start)>(dlsym(h, "ncclGroupStart"));
        r.group_end = reinterpret_cast<decltype(r.group_end)>(dlsym(h, "ncclGroupEnd"));
        r.err = reinterpret_cast<decltype(r.err)>(dlsym(h, "ncclGetErrorString"));
        r.all_reduce = reinterpret_cast<decltype(r.all_reduce)>(dlsym(h, "ncclAllReduce"));
        r.reduce = reinterpret_cast<decltype(r.reduce)>(dlsym(h, "ncclReduce"));
        r.reduce_scatter = reinterpret_cast<decltype(r.reduce_scatter)>(dlsym(h, "ncclReduceScatter"));
        r.ok = r.get_id && r.init_rank && r.destroy && r.send && r.recv && r.group_start && r.group_end && r.err;
        return r;
    }();
    return a.ok ? &a : nullptr;
}
}  // namespace

bool rccl_requested()
{
    static const bool v = [] {
        const char* e = getenv("MSX_TRANSPORT");
        return e && (strcmp(e, "rccl") == 0 || strcmp(e, "rccl_native") == 0);
    }();
    return v;
}

// MSX_TRANSPORT=rccl_native: (op, type) pairs that map onto RCCL's reductions
// run as ncclAllReduce / ncclReduce / ncclReduceScatter on the user's device
// buffers -- RCCL's ring/tree association, NOT the reference's: integer
// results are identical (two's-complement wrap), fp32/fp64 SUM and PROD agree
// within |y - y_ref| <= 2(p-1) 2^-p_mant sum_r |x_r|, MAX and
// MIN agree except where NaN / signed-zero ties decide.  Every other pair,
// host operands and ragged reduce_scatter counts keep the reference-order
// trees on the RCCL send/recv plane.
bool rccl_native_requested()
{
    static const bool v = [] {
        const char* e = getenv("MSX_TRANSPORT");
        return e && strcmp(e, "rccl_native") == 0;
    }();
    return v;
}

namespace {
bool rccl_map(int opidx, Kind k, ncclRedOp_t* op, ncclDataType_t* t)
{
    switch (opidx) {
    case O_SUM: *op = ncclSum; break;
    case O_PROD: *op = ncclProd; break;
    case O_MAX: *op = ncclMax; break;
    case O_MIN: *op = ncclMin; break;
    default: return false;      // O_SUM_WIDE too: its order is the engine's fused tree
    }
    switch (k) {
    case K_I8: *t = ncclInt8; return true;
    case K_U8: *t = ncclUint8; return true;
    case K_I32: *t = ncclInt32; return true;
    case K_U32: *t = ncclUint32; return true;
    case K_I64: *t = ncclInt64; return true;
    case K_U64: *t = ncclUint64; return true;
    case K_F32: *t = ncclFloat32; return true;
    case K_F64: *t = ncclFloat64; return true;
    default: return false;
    }
}

std::map<Transport*, ncclComm_t> g_rccl_comms;
std::map<Transport*, bool> g_rccl_refused;
// RCCL communicators of freed transports: retired, not destroyed.
// ncclCommDestroy would release RCCL's device buffers, and freeing uncached
// device memory corrupted later allocations on this stack.
std::vector<ncclComm_t> g_rccl_retired;
}  // namespace

// Called when `tp` is destroyed (engine worker, or finalize): a later
// transport may get the same address and must not find this one's state.
void rccl_forget(Transport* tp)
{
    auto it = g_rccl_comms.find(tp);
    if (it != g_rccl_comms.end()) {
        g_rccl_retired.push_back(it->second);
        g_rccl_comms.erase(it);
    }
    g_rccl_refused.erase(tp);
}

// Communicator for `tp` (collective on first use; nullptr = use IPC windows).
ncclComm_t rccl_comm(Transport* tp)
{
    auto& comms = g_rccl_comms;
    auto& refused = g_rccl_refused;
    auto it = comms.find(tp);
    if (it != comms.end()) return it->second;
    if (refused.count(tp)) return nullptr;
    const RcclApi* api = rccl_api();
    // every rank must take the same decision: agree on (api ok, device identity)
    struct Id { int32_t ok; int32_t dev; char bus[32]; };
    Id mine;
    memset(&mine, 0, sizeof(mine));
    mine.ok = api ? 1 : 0;
    (void)hipGetDevice(&mine.dev);
    (void)hipDeviceGetPCIBusId(mine.bus, sizeof(mine.bus), mine.dev);
    std::vector<Id> all((size_t)tp->size);
    if (tp->allgather(&mine, sizeof(mine), all.data()) != MPI_SUCCESS) { refused[tp] = true; return nullptr; }
    bool usable = true;
    for (int r = 0; r < tp->size; ++r) {
        usable = usable && all[r].ok;
        for (int q = 0; q < r; ++q) usable = usable && strncmp(all[r].bus, all[q].bus, sizeof(all[r].bus)) != 0;
    }
    if (!usable) {
        trace("rccl: not usable (library missing or ranks share a GPU); IPC windows in use");
        refused[tp] = true;
        return nullptr;
    }
    ncclUniqueId id;
    memset(&id, 0, sizeof(id));
    if (tp->rank == 0) api->get_id(&id);
    std::vector<ncclUniqueId> ids((size_t)tp->size);
    if (tp->allgather(&id, sizeof(id), ids.data()) != MPI_SUCCESS) { refused[tp] = true; return nullptr; }
    ncclComm_t comm = nullptr;
    ncclResult_t r = api->init_rank(&comm, tp->size, ids[0], tp->rank);
    trace("rccl: ncclCommInitRank rc=%d", (int)r);
    // Every rank must take the same plane: a rank whose init failed while its
    // peers' succeeded would run the IPC schedules against their RCCL calls and
    // hang both.  Agree on the outcome; any failure sends all to IPC windows.
    int32_t ok = r == ncclSuccess ? 1 : 0;
    std::vector<int32_t> oks((size_t)tp->size);
    if (tp->allgather(&ok, sizeof(ok), oks.data()) != MPI_SUCCESS) ok = 0;
    for (int32_t o : oks) ok = ok && o;
    if (!ok) {
        if (r == ncclSuccess) (void)api->destroy(comm);
        else set_error("ncclCommInitRank: %s", api->err(r));
        trace("rccl: a rank's ncclCommInitRank failed; IPC windows in use");
        refused[tp] = true;
        return nullptr;
    }
    comms[tp] = comm;
    return comm;
}

namespace {
// One ncclGroupStart/End batch of sends and receives (bytes), stream-ordered.
struct P2p {
    struct Op { bool send; void* buf; size_t n; int peer; };
    std::vector<Op> ops;
    void send(const void* b, size_t n, int peer) { if (n) ops.push_back({true, const_cast<void*>(b), n, peer}); }
    void recv(void* b, size_t n, int peer) { if (n) ops.push_back({false, b, n, peer}); }
    int run(ncclComm_t comm, hipStream_t s, const char* what)
    {
        if (ops.empty()) return MPI_SUCCESS;
        const RcclApi* api = rccl_api();
        ncclResult_t r = api->group_start();
        for (const Op& o : ops) {
            if (r != ncclSuccess) break;
            r = o.send ? api->send(o.buf, o.n, ncclUint8, o.peer, comm, s)
                       : api->recv(o.buf, o.n, ncclUint8, o.peer, comm, s);
        }
        ncclResult_t r2 = api->group_end();
        if (r == ncclSuccess) r = r2;
        if (r != ncclSuccess) { set_error("%s: %s", what, api->err(r)); return MPI_ERR_OTHER; }
        return MPI_SUCCESS;
    }
};
}  // namespace

int rccl_allreduce(ncclComm_t comm, Comm* c, const void* sendbuf, void* recvbuf, size_t count,
                   MPI_Datatype dt, const OpRef& op, int root, bool nbc)
{
    Transport* tp = c->tp;
    const int p = c->size, me = c->rank;
    const TypeInfo* ti = type_info(dt);
    const Kind k = ti->kind;
    const size_t esz = (size_t)ti->size;
    hipStream_t s = tp->stream();
    const char* src = static_cast<const char*>(sendbuf == MPI_IN_PLACE ? recvbuf : sendbuf);
    char* dst = static_cast<char*>(recvbuf);
    const bool want = (root < 0 || root == me);
    ncclRedOp_t nop;
    ncclDataType_t nty;
    const RcclApi* api = rccl_api();
    if (rccl_native_requested() && rccl_map(op.opidx, k, &nop, &nty) &&
        (root < 0 ? api->all_reduce != nullptr : api->reduce != nullptr)) {
        // Every rank takes this branch for a mappable pair (the pair is the
        // same on every rank), so no per-call agreement is needed: a rank
        // whose operands are host memory stages them through device scratch
        // (H2D, RCCL in place on the scratch, D2H) instead of leaving the
        // others in an RCCL collective alone.
        const bool sdev = classify(src).place == Place::Device;
        const bool ddev = !want || classify(dst).place == Place::Device;
        const char* in = src;
        char* out = want ? dst : const_cast<char*>(src);
        char* tmp = nullptr;
        int rc = MPI_SUCCESS;
        if (!sdev || !ddev) {
            tmp = dev_scratch(count * esz);
            if (!tmp) { set_error("allreduce: scratch allocation failed"); return MPI_ERR_NO_MEM; }
            rc = copy_async(tmp, src, count * esz, s);
            in = out = tmp;
        }
        if (rc != MPI_SUCCESS) return rc;
        ncclResult_t r = root < 0 ? api->all_reduce(in, out, count, nty, nop, comm, s)
                                  : api->reduce(in, out, count, nty, nop, root, comm, s);
        trace("rccl native %s: count=%zu staged=%d rc=%d", root < 0 ? "allreduce" : "reduce", count, tmp != nullptr,
              (int)r);
        if (r != ncclSuccess) {
            set_error("%s: %s", root < 0 ? "ncclAllReduce" : "ncclReduce", api->err(r));
            return MPI_ERR_OTHER;
        }
        if (tmp && want) rc = copy_async(dst, tmp, count * esz, s);
        return rc == MPI_SUCCESS ? sync_stream(s, root < 0 ? "allreduce" : "reduce") : rc;
    }
    const bool is_reduce = root >= 0;
    const int gate = gate_type_size(dt, nbc);
    const int algo = is_reduce ? reduce_algo(p, count, gate, true) : allreduce_algo(p, count, gate, true);
    const BufInfo bs = classify(src), bd = classify(dst);
    size_t qmax = (chunk_bytes() / (size_t)p) / esz;
    qmax -= qmax % 16;
    // scratch: [IN: p sub-slots of qmax, skewed apart (sub_skew)][OUT: p*qmax][stage: p*qmax]
    const size_t sub_b = qmax * esz, area = (size_t)p * sub_b;
    const size_t sub_s = sub_b + sub_skew(chunk_bytes() / (size_t)p);
    char* scratch = dev_scratch((size_t)p * sub_s + 2 * area);
    if (!scratch) { set_error("allreduce: scratch allocation failed"); return MPI_ERR_NO_MEM; }
    char* inb = scratch;
    char* outb = scratch + (size_t)p * sub_s;
    char* stage = outb + area;
    std::vector<char*> srcs((size_t)p);
    const int pof2 = pof2_floor(p);
    const int n = newrank_of(me, p);
    const int lineage = n >= 0 ? n : newrank_of(me + 1, p);
    int rc = MPI_SUCCESS;
    trace("rccl allreduce: count=%zu algo=%d qmax=%zu", count, algo, qmax);
    if (algo == A_RECURSIVE_DOUBLING || algo == A_BINOMIAL) {
        const RankTree t = (algo == A_BINOMIAL) ? tree_reduce_binomial(p, root) : tree_allreduce(p, lineage);
        for (size_t o = 0; o < count && rc == MPI_SUCCESS; o += qmax) {
            const size_t len = std::min(qmax, count - o);
            const char* mine = nullptr;
            rc = device_view(bs, src, o * esz, len * esz, stage, s, &mine);
            P2p x;
            for (int r = 0; r < p; ++r) {
                if (r == me) continue;
                if (root < 0 || r == root) x.send(mine, len * esz, r);
                if (want) x.recv(inb + (size_t)r * sub_s, len * esz, r);
            }
            if (rc == MPI_SUCCESS) rc = x.run(comm, s, "allreduce exchange");
            if (rc == MPI_SUCCESS && want) {
                for (int r = 0; r < p; ++r) srcs[r] = (r == me) ? const_cast<char*>(mine) : inb + (size_t)r * sub_s;
                char* out = bd.place == Place::Device ? static_cast<char*>(bd.dev) + o * esz : outb;
                rc = run_rank_tree(op.opidx, k, t, srcs, esz, 0, len, out, s);
                if (rc == MPI_SUCCESS && out == outb) rc = copy_async(dst + o * esz, out, len * esz, s);
            }
        }
        return rc == MPI_SUCCESS ? sync_stream(s, "allreduce") : rc;
    }
    const size_t ce = (size_t)p * qmax;
    for (size_t o = 0; o < count && rc == MPI_SUCCESS; o += ce) {
        const size_t len = std::min(ce, count - o);
        const size_t q = (len + p - 1) / p;
        const size_t qv = (q + 15) & ~(size_t)15;
        auto lo_of = [&](int r) { return std::min(len, (size_t)r * qv); };
        auto hi_of = [&](int r) { return std::min(len, (size_t)(r + 1) * qv); };
        const size_t plo = lo_of(me), phi = hi_of(me);
        const char* mine = nullptr;
        rc = device_view(bs, src, o * esz, len * esz, stage, s, &mine);
        P2p x;                                        // reduce-scatter as all-to-all
        for (int r = 0; r < p; ++r) {
            if (r == me) continue;
            x.send(mine + lo_of(r) * esz, (hi_of(r) - lo_of(r)) * esz, r);
            x.recv(inb + (size_t)r * sub_s, (phi - plo) * esz, r);
        }
        if (rc == MPI_SUCCESS) rc = x.run(comm, s, "allreduce scatter");
        for (int r = 0; r < p; ++r) srcs[r] = (r == me) ? const_cast<char*>(mine) + plo * esz : inb + (size_t)r * sub_s;
        char* outp = (want && bd.place == Place::Device) ? static_cast<char*>(bd.dev) + o * esz : outb;
        for (size_t e0 = plo; e0 < phi && rc == MPI_SUCCESS;) {
            const size_t ge = o + e0;
            const size_t rs = count / (size_t)pof2;
            const int j = rs ? (int)std::min((size_t)pof2 - 1, ge / rs) : pof2 - 1;
            size_t bst, bl;
            allreduce_block(p, count, j, &bst, &bl);
            const size_t e1 = std::min(phi, bst + bl - o);
            const int owner = allreduce_block_owner(p, j);
            const RankTree t = !is_reduce ? tree_allreduce(p, owner)
                                          : (nbc ? tree_ireduce_rsag(p, owner, root) : tree_reduce_rsag(p, owner));
            rc = run_rank_tree(op.opidx, k, t, srcs, esz, e0 - plo, e1 - e0, outp + e0 * esz, s);
            e0 = e1;
        }
        P2p g;                                        // allgather (or gather at root)
        for (int r = 0; r < p; ++r) {
            if (r == me) continue;
            if (root < 0 || r == root) g.send(outp + plo * esz, (phi - plo) * esz, r);
            if (want) g.recv(outp + lo_of(r) * esz, (hi_of(r) - lo_of(r)) * esz, r);
        }
        if (rc == MPI_SUCCESS) rc = g.run(comm, s, "allreduce gather");
        if (rc == MPI_SUCCESS && want && outp == outb) rc = copy_async(dst + o * esz, outb, len * esz, s);
    }
    return rc == MPI_SUCCESS ? sync_stream(s, "allreduce") : rc;
}

int rccl_reduce_scatter(ncclComm_t comm, Comm* c, const void* sendbuf, void* recvbuf, const int* recvcounts,
                        MPI_Datatype dt, const OpRef& op)
{
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
    const bool in_place = (sendbuf == MPI_IN_PLACE);
    const char* src = static_cast<const char*>(in_place ? recvbuf : sendbuf);
    const Kind k = type_info(dt)->kind;
    hipStream_t s = tp->stream();
    ncclRedOp_t nop;
    ncclDataType_t nty;
    const RcclApi* api = rccl_api();
    if (rccl_native_requested() && api->reduce_scatter && rccl_map(op.opidx, k, &nop, &nty) &&
        maxcnt * (size_t)p == total) {
        // equal blocks (recvcounts are the same on every rank by MPI rule):
        // ncclReduceScatter.  Taken by every rank alike (no per-call
        // agreement): host operands are staged through device scratch, and in
        // place my block moves to recvbuf[0]
        const bool sdev = classify(src).place == Place::Device, ddev = classify(recvbuf).place == Place::Device;
        const char* in = src;
        void* out = recvbuf;
        char* tmp = nullptr;
        int rc = MPI_SUCCESS;
        if (!sdev || !ddev) {
            tmp = dev_scratch((total + maxcnt) * esz);          // [input][my block]
            if (!tmp) { set_error("reduce_scatter: scratch allocation failed"); return MPI_ERR_NO_MEM; }
            rc = copy_async(tmp, src, total * esz, s);
            in = tmp;
            out = tmp + total * esz;
        } else if (in_place && me != 0 && maxcnt) {
            tmp = dev_scratch(maxcnt * esz);      // RCCL's in-place form wants recvbuf + rank*count
            if (!tmp) { set_error("reduce_scatter: scratch allocation failed"); return MPI_ERR_NO_MEM; }
            out = tmp;
        }
        if (rc != MPI_SUCCESS) return rc;
        ncclResult_t r = api->reduce_scatter(in, out, maxcnt, nty, nop, comm, s);
        trace("rccl native reduce_scatter: count=%zu staged=%d rc=%d", maxcnt, (!sdev || !ddev), (int)r);
        if (r != ncclSuccess) { set_error("ncclReduceScatter: %s", api->err(r)); return MPI_ERR_OTHER; }
        if (out != recvbuf) rc = copy_async(recvbuf, out, maxcnt * esz, s);
        return rc == MPI_SUCCESS ? sync_stream(s, "reduce_scatter") : rc;
    }
    size_t qe = (chunk_bytes() / (size_t)p) / esz;
    qe -= qe % 16;
    const int algo = reduce_scatter_algo(p, total, gate_type_size(dt, false), op.commutative);
    const int n = newrank_of(me, p);
    const RankTree t = (algo == A_RS_PAIRWISE) ? tree_pairwise(p, me)
                                               : tree_reduce_scatter(p, n >= 0 ? n : newrank_of(me + 1, p));
    const size_t mycnt = (size_t)recvcounts[me];
    const BufInfo bs = classify(src), bd = classify(recvbuf);
    char* dst = static_cast<char*>(recvbuf);
    // scratch: [IN: p sub-slots of qe, skewed apart][OUT: qe][stage: p*qe][hold: mycnt if in place]
    const size_t sub_b = qe * esz, area = (size_t)p * sub_b;
    const size_t sub_s = sub_b + sub_skew(chunk_bytes() / (size_t)p);
    const size_t hold_b = in_place ? mycnt * esz : 0;
    char* scratch = dev_scratch((size_t)p * sub_s + area + sub_b + hold_b);
    if (!scratch) { set_error("reduce_scatter: scratch allocation failed"); return MPI_ERR_NO_MEM; }
    char* inb = scratch;
    char* outb = scratch + (size_t)p * sub_s;
    char* stage = outb + sub_b;
    char* hold = stage + area;
    std::vector<char*> srcs((size_t)p);
    int rc = MPI_SUCCESS;
    trace("rccl reduce_scatter: total=%zu algo=%d round=%zu", total, algo, qe);
    for (size_t o = 0; o < maxcnt && rc == MPI_SUCCESS; o += qe) {
        P2p x;
        const char* myseg = nullptr;
        for (int r = 0; r < p && rc == MPI_SUCCESS; ++r) {
            const size_t cnt = (size_t)recvcounts[r];
            if (o >= cnt) continue;
            const size_t len = std::min(qe, cnt - o);
            const char* v = nullptr;
            rc = device_view(bs, src, (disp[r] + o) * esz, len * esz, stage + (size_t)r * sub_b, s, &v);
            if (r == me) myseg = v;
            else x.send(v, len * esz, r);
        }
        const size_t len = o < mycnt ? std::min(qe, mycnt - o) : 0;
        for (int r = 0; r < p; ++r)
            if (r != me) x.recv(inb + (size_t)r * sub_s, len * esz, r);
        if (rc == MPI_SUCCESS) rc = x.run(comm, s, "reduce_scatter exchange");
        if (rc == MPI_SUCCESS && len) {
            for (int r = 0; r < p; ++r) srcs[r] = (r == me) ? const_cast<char*>(myseg) : inb + (size_t)r * sub_s;
            char* out = in_place ? hold + o * esz
                                 : (bd.place == Place::Device ? static_cast<char*>(bd.dev) + o * esz : outb);
            rc = run_rank_tree(op.opidx, k, t, srcs, esz, 0, len, out, s);
            if (rc == MPI_SUCCESS && out == outb) rc = copy_async(dst + o * esz, out, len * esz, s);
        }
    }
    if (rc == MPI_SUCCESS && in_place && mycnt) rc = copy_async(recvbuf, hold, mycnt * esz, s);
    return rc == MPI_SUCCESS ? sync_stream(s, "reduce_scatter") : rc;
}

const char* engine_transport_name(Transport* tp)
{
    if (!tp) return "self";
    if (!worker().submit([tp]() -> int { return g_rccl_comms.count(tp) ? 1 : 0; }).get()) return "ipc";
    return rccl_native_requested() ? "rccl_native" : "rccl";
}

}  // namespace msx
