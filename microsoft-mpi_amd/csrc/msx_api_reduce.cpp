// msx_api_reduce.cpp — MPI_Reduce_local, the reduction collectives, the scans
// and their non-blocking forms (argument-validation order: see msx_api.cpp).
#include <algorithm>
#include <stdlib.h>
#include <vector>

#include "msx_api.h"
#include "msx_dtype.h"
#include "msx_kernels.h"
#include "msx_transport.h"

using namespace msx;

// ===========================================================================
// MPI_Reduce_local (api/mpi_reduce.cpp:304-385)
// ===========================================================================
MSX_EXPORT int MPI_Reduce_local(const void* inbuf, void* inoutbuf, int count,
                                MPI_Datatype datatype, MPI_Op op)
{
    MSX_REQUIRE_INIT("MPI_Reduce_local");
    if (count == 0) return MPI_SUCCESS;             // :319-322, before any check
    OpRef r;
    int rc = v_op(op, datatype, &r);                // :324
    if (rc == MPI_SUCCESS && inbuf == MPI_IN_PLACE) { set_error("inbuf is MPI_IN_PLACE"); rc = MPI_ERR_BUFFER; }
    if (rc == MPI_SUCCESS && inoutbuf == MPI_IN_PLACE) { set_error("inoutbuf is MPI_IN_PLACE"); rc = MPI_ERR_BUFFER; }
    if (rc == MPI_SUCCESS) rc = v_dtype_any(inbuf, count, datatype);   // :343
    if (rc == MPI_SUCCESS && inbuf == inoutbuf) { set_error("inbuf aliases inoutbuf"); rc = MPI_ERR_BUFFER; }
    // MSX_REDUCE_LOCAL_GPUS=k (k = 0: every GPU of the node): host operands
    // split over k GPUs' PCIe links (reduce_local_multi); for single-process
    // use -- in a job with one rank per GPU each rank would use them all
    static const int multi = [] {
        const char* e = getenv("MSX_REDUCE_LOCAL_GPUS");
        return e ? atoi(e) : 1;
    }();
    if (rc == MPI_SUCCESS && multi != 1 && r.opidx != O_NULL && type_info(datatype))
        rc = reduce_local_multi(r.opidx, type_info(datatype)->kind, inbuf, inoutbuf, (size_t)count, multi);
    else if (rc == MPI_SUCCESS)
        rc = local_combine(r, datatype, inbuf, inoutbuf, (size_t)count);
    return err_return(nullptr, "MPI_Reduce_local", rc);
}

// ===========================================================================
// reduction collectives
// ===========================================================================
namespace {

// api/mpi_reduce.cpp:1073-1160: recvbuf / sendbuf rules of MPI_Allreduce
// (MPI_IN_PLACE is not allowed on an intercommunicator)
int v_allreduce_bufs(Comm* c, const void* sendbuf, void* recvbuf, int count, MPI_Datatype datatype)
{
    if (recvbuf == MPI_IN_PLACE) { set_error("recvbuf is MPI_IN_PLACE"); return MPI_ERR_BUFFER; }
    if (sendbuf == MPI_IN_PLACE) {
        if (c->inter) { set_error("**sendbuf_inplace on an intercommunicator"); return MPI_ERR_BUFFER; }
        return MPI_SUCCESS;
    }
    int rc = v_buffer(datatype, sendbuf, count);
    if (rc == MPI_SUCCESS && sendbuf == recvbuf) { set_error("sendbuf aliases recvbuf"); rc = MPI_ERR_BUFFER; }
    return rc;
}

// api/mpi_reduce.cpp:46-273: MPI_Reduce's checks; on an intercommunicator the
// root is MPI_ROOT (receives), MPI_PROC_NULL (does nothing) or a remote rank
// (sends).  *skip: nothing to do on this process.
int v_reduce(Comm* c, const void* sendbuf, void* recvbuf, int count, MPI_Datatype datatype, MPI_Op op, int root,
             OpRef* r, bool* skip)
{
    *skip = false;
    if (c->inter) {
        if (root == MPI_PROC_NULL) { *skip = true; return MPI_SUCCESS; }
        if (root == MPI_ROOT) {
            int rc = v_dtype_any(recvbuf, count, datatype);
            if (rc == MPI_SUCCESS) rc = v_op(op, datatype, r);
            return rc == MPI_SUCCESS ? v_no_device_op_inter(c, *r) : rc;
        }
        if (root < 0 || root >= (int)c->remote_lpid.size()) { set_error("invalid root %d", root); return MPI_ERR_ROOT; }
        if (count > 0 && sendbuf == MPI_IN_PLACE) { set_error("**sendbuf_inplace"); return MPI_ERR_BUFFER; }
        int rc = v_dtype_any(sendbuf, count, datatype);
        if (rc == MPI_SUCCESS) rc = v_op(op, datatype, r);
        return rc == MPI_SUCCESS ? v_no_device_op_inter(c, *r) : rc;
    }
    if (root < 0 || root >= c->size) { set_error("invalid root %d", root); return MPI_ERR_ROOT; }
    int rc = v_dtype_any(sendbuf, count, datatype);
    if (rc == MPI_SUCCESS) rc = v_op(op, datatype, r);
    if (rc != MPI_SUCCESS) return rc;
    if (c->rank == root) {
        if (recvbuf == MPI_IN_PLACE) { set_error("recvbuf is MPI_IN_PLACE"); return MPI_ERR_BUFFER; }
        rc = v_buffer(datatype, recvbuf, count);
        if (rc == MPI_SUCCESS && count > 0 && sendbuf == recvbuf) { set_error("sendbuf aliases recvbuf"); rc = MPI_ERR_BUFFER; }
    } else if (count > 0 && sendbuf == MPI_IN_PLACE) {
        set_error("sendbuf is MPI_IN_PLACE on a non-root rank");
        rc = MPI_ERR_BUFFER;
    }
    return rc;
}

int run_reduce(Comm* c, const void* sendbuf, void* recvbuf, size_t n, MPI_Datatype datatype, const OpRef& r, int root,
               bool nbc)
{
    if (n == 0) return MPI_SUCCESS;
    return c->inter ? engine_inter_reduce(c, sendbuf, recvbuf, n, datatype, r, root)
                    : coll_reduce(c, sendbuf, recvbuf, n, datatype, r, root, nbc);
}

int run_reduce_scatter(Comm* c, const void* sendbuf, void* recvbuf, const int* counts, MPI_Datatype datatype,
                       const OpRef& r)
{
    return c->inter ? engine_inter_reduce_scatter(c, sendbuf, recvbuf, counts, datatype, r)
                    : coll_reduce_scatter(c, sendbuf, recvbuf, counts, datatype, r);
}

// The request of a non-blocking form, checked right after the communicator
int v_request(MPI_Request* request)
{
    if (request == nullptr) { set_error("null request"); return MPI_ERR_ARG; }
    *request = MPI_REQUEST_NULL;
    return MPI_SUCCESS;
}

// One body per collective: nonblocking = false is the blocking call (request
// unused), true its MPI_I* form.  MPI_Allreduce with count == 0 returns after
// validation; MPI_Iallreduce still creates a request.
int allreduce_common(const char* fn, const void* sendbuf, void* recvbuf, int count, MPI_Datatype datatype, MPI_Op op,
                     MPI_Comm comm, MPI_Request* request = nullptr, bool nonblocking = false)
{
    MSX_REQUIRE_INIT(fn);
    Comm* c;
    OpRef r;
    int rc = v_comm(comm, &c);
    if (rc == MPI_SUCCESS && nonblocking) rc = v_request(request);
    if (rc == MPI_SUCCESS) rc = v_dtype_any(recvbuf, count, datatype);
    if (rc == MPI_SUCCESS) rc = v_op(op, datatype, &r);
    if (rc == MPI_SUCCESS) rc = v_no_device_op_inter(c, r);
    if (rc == MPI_SUCCESS && count > 0) rc = v_allreduce_bufs(c, sendbuf, recvbuf, count, datatype);
    const size_t n = (size_t)count;
    if (rc == MPI_SUCCESS && !nonblocking && n > 0) {
        rc = c->inter ? engine_inter_allreduce(c, sendbuf, recvbuf, n, datatype, r)
                      : coll_allreduce(c, sendbuf, recvbuf, n, datatype, r, force_async());
    } else if (rc == MPI_SUCCESS && nonblocking && c->inter) {
        rc = request_start_generic(c, [=] {
            return n ? engine_inter_allreduce(c, sendbuf, recvbuf, n, datatype, r) : MPI_SUCCESS;
        }, request, datatype);
    } else if (rc == MPI_SUCCESS && nonblocking) {
        rc = request_start_allreduce(c, sendbuf, recvbuf, n, datatype, r, request);
    }
    return err_return(c, fn, rc);
}

// With nothing to do on this process (v_reduce's skip) MPI_Ireduce runs with n = 0.
int reduce_common(const char* fn, const void* sendbuf, void* recvbuf, int count, MPI_Datatype datatype, MPI_Op op,
                  int root, MPI_Comm comm, MPI_Request* request = nullptr, bool nonblocking = false)
{
    MSX_REQUIRE_INIT(fn);
    Comm* c;
    OpRef r;
    bool skip = false;
    int rc = v_comm(comm, &c);
    if (rc == MPI_SUCCESS && nonblocking) rc = v_request(request);
    if (rc == MPI_SUCCESS) rc = v_reduce(c, sendbuf, recvbuf, count, datatype, op, root, &r, &skip);
    if (rc == MPI_SUCCESS && nonblocking) {
        const size_t n = skip ? 0 : (size_t)count;
        rc = request_start_generic(c, [=] { return run_reduce(c, sendbuf, recvbuf, n, datatype, r, root, true); },
                                   request, datatype);
    } else if (rc == MPI_SUCCESS && !skip) {
        rc = run_reduce(c, sendbuf, recvbuf, (size_t)count, datatype, r, root, force_async());
    }
    return err_return(c, fn, rc);
}

int validate_reduce_scatter(Comm* c, const void* sendbuf, void* recvbuf, const int* recvcounts,
                            MPI_Datatype datatype, MPI_Op op, OpRef* r)
{
    if (!recvcounts) { set_error("null recvcounts"); return MPI_ERR_ARG; }
    int sentinel = 0;
    for (int i = 0; i < c->size; ++i) {
        if (recvcounts[i] < 0) { set_error("negative recvcount %d", recvcounts[i]); return MPI_ERR_COUNT; }
        sentinel |= recvcounts[i];   // the reference's OR trick (mpi_reduce.cpp:833-847)
    }
    int rc = v_dtype_any(sendbuf, sentinel, datatype);
    if (rc == MPI_SUCCESS) rc = v_op(op, datatype, r);
    if (rc == MPI_SUCCESS) rc = v_no_device_op_inter(c, *r);
    if (rc == MPI_SUCCESS && recvcounts[c->rank] > 0) {
        if (recvbuf == MPI_IN_PLACE) { set_error("recvbuf is MPI_IN_PLACE"); rc = MPI_ERR_BUFFER; }
        else if (sendbuf != MPI_IN_PLACE) {
            rc = v_buffer(datatype, recvbuf, recvcounts[c->rank]);
            if (rc == MPI_SUCCESS && sendbuf == recvbuf) { set_error("sendbuf aliases recvbuf"); rc = MPI_ERR_BUFFER; }
        } else if (c->inter) {                // mpi_reduce.cpp:893-897
            set_error("**sendbuf_inplace on an intercommunicator");
            rc = MPI_ERR_BUFFER;
        }
    }
    return rc;
}

// block_count: null for MPI_(I)reduce_scatter over recvcounts; else the _block
// forms' one count, checked and spread over the ranks before the validation.
int reduce_scatter_common(const char* fn, const void* sendbuf, void* recvbuf, const int* recvcounts,
                          const int* block_count, MPI_Datatype datatype, MPI_Op op, MPI_Comm comm,
                          MPI_Request* request = nullptr, bool nonblocking = false)
{
    MSX_REQUIRE_INIT(fn);
    Comm* c;
    OpRef r;
    int rc = v_comm(comm, &c);
    if (rc == MPI_SUCCESS && nonblocking) rc = v_request(request);
    if (rc == MPI_SUCCESS && block_count && *block_count < 0) { set_error("negative recvcount"); rc = MPI_ERR_COUNT; }
    std::vector<int> counts;
    if (rc == MPI_SUCCESS && block_count) {
        counts.assign((size_t)c->size, *block_count);
        recvcounts = counts.data();
    }
    if (rc == MPI_SUCCESS) rc = validate_reduce_scatter(c, sendbuf, recvbuf, recvcounts, datatype, op, &r);
    if (rc == MPI_SUCCESS && nonblocking) {
        if (!block_count) counts.assign(recvcounts, recvcounts + c->size);   // the request keeps its own copy
        rc = request_start_generic(c, [=] {
            return run_reduce_scatter(c, sendbuf, recvbuf, counts.data(), datatype, r);
        }, request, datatype);
    } else if (rc == MPI_SUCCESS) {
        rc = run_reduce_scatter(c, sendbuf, recvbuf, recvcounts, datatype, r);
    }
    return err_return(c, fn, rc);
}

// request == nullptr: blocking MPI_(Ex)scan; else MPI_I(ex)scan
// (api/mpi_reduce.cpp:1920-2068 validate like the blocking forms)
int scan_common(const char* fn, const void* sendbuf, void* recvbuf, int count, MPI_Datatype datatype,
                MPI_Op op, MPI_Comm comm, bool exclusive, MPI_Request* request = nullptr,
                bool nonblocking = false)
{
    MSX_REQUIRE_INIT(fn);
    Comm* c;
    OpRef r;
    int rc = v_intracomm(comm, &c);      // scans are defined on intracommunicators only
    if (rc == MPI_SUCCESS && nonblocking) rc = v_request(request);
    if (rc == MPI_SUCCESS) rc = v_dtype_any(recvbuf, count, datatype);
    if (rc == MPI_SUCCESS) rc = v_op(op, datatype, &r);
    if (rc == MPI_SUCCESS) rc = v_no_sum_wide(r, "MPI_Scan / MPI_Exscan (their steps exchange rounded partials)");
    if (rc == MPI_SUCCESS && count > 0) {
        if (recvbuf == MPI_IN_PLACE) { set_error("recvbuf is MPI_IN_PLACE"); rc = MPI_ERR_BUFFER; }
        else if (sendbuf != MPI_IN_PLACE) {
            rc = v_buffer(datatype, sendbuf, count);
            if (rc == MPI_SUCCESS && sendbuf == recvbuf) { set_error("sendbuf aliases recvbuf"); rc = MPI_ERR_BUFFER; }
        }
    }
    if (rc == MPI_SUCCESS && nonblocking) {
        const size_t n = (size_t)count;
        rc = request_start_generic(c, [=] {
            return n ? coll_scan(c, sendbuf, recvbuf, n, datatype, r, exclusive) : MPI_SUCCESS;
        }, request, datatype);
    } else if (rc == MPI_SUCCESS && count > 0) {
        rc = coll_scan(c, sendbuf, recvbuf, (size_t)count, datatype, r, exclusive);
    }
    return err_return(c, fn, rc);
}

}  // namespace

MSX_EXPORT int MPI_Allreduce(const void* sendbuf, void* recvbuf, int count, MPI_Datatype datatype,
                             MPI_Op op, MPI_Comm comm)
{
    return allreduce_common("MPI_Allreduce", sendbuf, recvbuf, count, datatype, op, comm);
}

MSX_EXPORT int MPI_Reduce(const void* sendbuf, void* recvbuf, int count, MPI_Datatype datatype,
                          MPI_Op op, int root, MPI_Comm comm)
{
    return reduce_common("MPI_Reduce", sendbuf, recvbuf, count, datatype, op, root, comm);
}

MSX_EXPORT int MPI_Reduce_scatter(const void* sendbuf, void* recvbuf, const int recvcounts[],
                                  MPI_Datatype datatype, MPI_Op op, MPI_Comm comm)
{
    return reduce_scatter_common("MPI_Reduce_scatter", sendbuf, recvbuf, recvcounts, nullptr, datatype, op, comm);
}

MSX_EXPORT int MPI_Reduce_scatter_block(const void* sendbuf, void* recvbuf, int recvcount,
                                        MPI_Datatype datatype, MPI_Op op, MPI_Comm comm)
{
    return reduce_scatter_common("MPI_Reduce_scatter_block", sendbuf, recvbuf, nullptr, &recvcount, datatype, op,
                                 comm);
}

MSX_EXPORT int MPI_Scan(const void* sendbuf, void* recvbuf, int count, MPI_Datatype datatype,
                        MPI_Op op, MPI_Comm comm)
{
    return scan_common("MPI_Scan", sendbuf, recvbuf, count, datatype, op, comm, false);
}

MSX_EXPORT int MPI_Exscan(const void* sendbuf, void* recvbuf, int count, MPI_Datatype datatype,
                          MPI_Op op, MPI_Comm comm)
{
    return scan_common("MPI_Exscan", sendbuf, recvbuf, count, datatype, op, comm, true);
}

MSX_EXPORT int MPI_Iscan(const void* sendbuf, void* recvbuf, int count, MPI_Datatype datatype,
                         MPI_Op op, MPI_Comm comm, MPI_Request* request)
{
    return scan_common("MPI_Iscan", sendbuf, recvbuf, count, datatype, op, comm, false, request, true);
}

MSX_EXPORT int MPI_Iexscan(const void* sendbuf, void* recvbuf, int count, MPI_Datatype datatype,
                           MPI_Op op, MPI_Comm comm, MPI_Request* request)
{
    return scan_common("MPI_Iexscan", sendbuf, recvbuf, count, datatype, op, comm, true, request, true);
}

// ---- non-blocking variants: stream-ordered requests -----------------------
MSX_EXPORT int MPI_Iallreduce(const void* sendbuf, void* recvbuf, int count, MPI_Datatype datatype,
                              MPI_Op op, MPI_Comm comm, MPI_Request* request)
{
    return allreduce_common("MPI_Iallreduce", sendbuf, recvbuf, count, datatype, op, comm, request, true);
}

MSX_EXPORT int MPI_Ireduce(const void* sendbuf, void* recvbuf, int count, MPI_Datatype datatype,
                           MPI_Op op, int root, MPI_Comm comm, MPI_Request* request)
{
    return reduce_common("MPI_Ireduce", sendbuf, recvbuf, count, datatype, op, root, comm, request, true);
}

MSX_EXPORT int MPI_Ireduce_scatter(const void* sendbuf, void* recvbuf, const int recvcounts[],
                                   MPI_Datatype datatype, MPI_Op op, MPI_Comm comm,
                                   MPI_Request* request)
{
    return reduce_scatter_common("MPI_Ireduce_scatter", sendbuf, recvbuf, recvcounts, nullptr, datatype, op, comm,
                                 request, true);
}

MSX_EXPORT int MPI_Ireduce_scatter_block(const void* sendbuf, void* recvbuf, int recvcount,
                                         MPI_Datatype datatype, MPI_Op op, MPI_Comm comm,
                                         MPI_Request* request)
{
    return reduce_scatter_common("MPI_Ireduce_scatter_block", sendbuf, recvbuf, nullptr, &recvcount, datatype, op,
                                 comm, request, true);
}

// ---- PMPI_ profiling aliases (dll/msmpi.def) --------------------------------
MSX_ALIAS(MPI_Reduce_local) int PMPI_Reduce_local(const void*, void*, int, MPI_Datatype, MPI_Op);
MSX_ALIAS(MPI_Reduce) int PMPI_Reduce(const void*, void*, int, MPI_Datatype, MPI_Op, int, MPI_Comm);
MSX_ALIAS(MPI_Allreduce) int PMPI_Allreduce(const void*, void*, int, MPI_Datatype, MPI_Op, MPI_Comm);
MSX_ALIAS(MPI_Reduce_scatter_block) int PMPI_Reduce_scatter_block(const void*, void*, int, MPI_Datatype, MPI_Op, MPI_Comm);
MSX_ALIAS(MPI_Reduce_scatter) int PMPI_Reduce_scatter(const void*, void*, const int[], MPI_Datatype, MPI_Op, MPI_Comm);
MSX_ALIAS(MPI_Iallreduce) int PMPI_Iallreduce(const void*, void*, int, MPI_Datatype, MPI_Op, MPI_Comm, MPI_Request*);
MSX_ALIAS(MPI_Iscan) int PMPI_Iscan(const void*, void*, int, MPI_Datatype, MPI_Op, MPI_Comm, MPI_Request*);
MSX_ALIAS(MPI_Iexscan) int PMPI_Iexscan(const void*, void*, int, MPI_Datatype, MPI_Op, MPI_Comm, MPI_Request*);
MSX_ALIAS(MPI_Scan) int PMPI_Scan(const void*, void*, int, MPI_Datatype, MPI_Op, MPI_Comm);
MSX_ALIAS(MPI_Exscan) int PMPI_Exscan(const void*, void*, int, MPI_Datatype, MPI_Op, MPI_Comm);
MSX_ALIAS(MPI_Ireduce) int PMPI_Ireduce(const void*, void*, int, MPI_Datatype, MPI_Op, int, MPI_Comm, MPI_Request*);
MSX_ALIAS(MPI_Ireduce_scatter_block) int PMPI_Ireduce_scatter_block(const void*, void*, int, MPI_Datatype, MPI_Op,
                                                                    MPI_Comm, MPI_Request*);
MSX_ALIAS(MPI_Ireduce_scatter) int PMPI_Ireduce_scatter(const void*, void*, const int*, MPI_Datatype, MPI_Op,
                                                        MPI_Comm, MPI_Request*);
