// msx_api.cpp — MPI-2.2 C entry points of the reduction path: the validators and
// the error return of every entry-point unit (msx_api.h), environment,
// communicators, error handlers, operations and their pool.  The rest is in
// msx_api_reduce.cpp, _request.cpp, _rma.cpp (one-sided) and _ext.cpp (msx_* ABI).
//
// Each function keeps the reference's argument-validation ORDER, because the
// first failing check decides which error class a caller sees:
//   MPI_Reduce_local           api/mpi_reduce.cpp:304-385
//   MPI_Reduce                 api/mpi_reduce.cpp:46-273
//   MPI_Allreduce              api/mpi_reduce.cpp:1246-1410
//   MPI_Reduce_scatter(_block) api/mpi_reduce.cpp:422-997
//   MPI_Iallreduce / I*        api/mpi_reduce.cpp:1445-1591, 617-790
//   MPI_Scan / MPI_Exscan      api/mpi_reduce.cpp:1626-1900
//   MPI_Op_create/free/commutative  api/mpi_op.cpp:48-260
//   validators MpiaOpValidate / MpiaDatatypeValidate  api/mpi_api.h:113-212, 707-775
//   error return               mpid/error.cpp:85-134 (ERRORS_ARE_FATAL default)
#include <algorithm>
#include <chrono>
#include <mutex>
#include <thread>
#include <unistd.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#include "msx_api.h"
#include "msx_dtype.h"
#include "msx_transport.h"

using namespace msx;

namespace {

// ---------------------------------------------------------------------------
// user ops: MPID_Op pool for HANDLE_TYPE_DIRECT op handles (include/op.h:82-134)
// ---------------------------------------------------------------------------
struct UserOp {
    MPI_User_function* fn = nullptr;
    bool commute = true;
    bool live = false;
    MSX_Device_function* dev_fn = nullptr;   // msx_op_create_device: fn is null
    void* dev_state = nullptr;
    MSX_Device_tree_function* dev_tree = nullptr;   // msx_op_create_device_tree
};
std::mutex g_op_mu;
std::vector<UserOp> g_user_ops;
constexpr int kUserOpBase = (int)0x98000000;   // type DIRECT (2) | kind MPID_OP (6)

// The handle of `u` in the first free slot of the pool (MPI_Op_create and the
// device op constructors).
MPI_Op op_pool_add(const UserOp& u)
{
    std::lock_guard<std::mutex> g(g_op_mu);
    size_t idx = 0;
    while (idx < g_user_ops.size() && g_user_ops[idx].live) ++idx;
    if (idx == g_user_ops.size()) g_user_ops.push_back(UserOp{});
    g_user_ops[idx] = u;
    return kUserOpBase | (int)idx;
}

// A user op whose function enqueues its combine on a HIP stream (msx.h): the
// same MPID_Op pool and handle layout as MPI_Op_create.
int device_op_create(MSX_Device_function* fn, MSX_Device_tree_function* tree_fn, int commute, void* state, MPI_Op* op)
{
    if (fn == nullptr) { set_error("null device function"); return MPI_ERR_ARG; }
    if (op == nullptr) { set_error("null op"); return MPI_ERR_ARG; }
    *op = op_pool_add(UserOp{nullptr, commute != 0, true, fn, state, tree_fn});
    return MPI_SUCCESS;
}

const char* class_string(int cls)
{
    switch (cls) {
    case MPI_SUCCESS: return "No MPI error";
    case MPI_ERR_BUFFER: return "Invalid buffer pointer";
    case MPI_ERR_COUNT: return "Invalid count argument";
    case MPI_ERR_TYPE: return "Invalid datatype argument";
    case MPI_ERR_TAG: return "Invalid tag argument";
    case MPI_ERR_COMM: return "Invalid communicator";
    case MPI_ERR_RANK: return "Invalid rank";
    case MPI_ERR_ROOT: return "Invalid root";
    case MPI_ERR_GROUP: return "Invalid group";
    case MPI_ERR_OP: return "Invalid MPI_Op";
    case MPI_ERR_ARG: return "Invalid argument";
    case MPI_ERR_UNKNOWN: return "Unknown error";
    case MPI_ERR_TRUNCATE: return "Message truncated";
    case MPI_ERR_OTHER: return "Other MPI error";
    case MPI_ERR_INTERN: return "Internal MPI error";
    case MPI_ERR_REQUEST: return "Invalid MPI_Request";
    case MPI_ERR_NO_MEM: return "Out of memory";
    case MPI_ERR_INFO: return "Invalid info argument";
    case MPI_ERR_WIN: return "Invalid win argument";
    case MPI_ERR_RMA_SYNC: return "Wrong synchronization of RMA calls";
    case MPI_ERR_SIZE: return "Invalid size argument";
    case MPI_ERR_DISP: return "Invalid disp argument";
    default: return "Unknown error class";
    }
}

bool dtype_known(MPI_Datatype dt) { return type_size(dt) >= 0; }

}  // namespace

namespace msx {

void not_initialized_exit(const char* fn)
{
    // MpiaIsInitializedOrExit -> MPIR_Err_preOrPostInit (api/mpi_api.h:27)
    fprintf(stderr,
            "Fatal error in %s: Attempting to use an MPI routine %s MPI_Init\n", fn,
            is_finalized() ? "after finalizing" : "before initializing");
    fflush(stderr);
    exit(1);
}

// MPIR_Err_return_comm (mpid/error.cpp:85-134): default handler is the one on
// MPI_COMM_WORLD; ERRORS_ARE_FATAL aborts the job.
int err_return_h(MPI_Errhandler h, const char* fn, int code)
{
    if (code == MPI_SUCCESS) return code;
    if (h == MPI_ERRORS_ARE_FATAL) {
        const char* detail = last_error();
        fprintf(stderr, "Fatal error in %s: %s, error stack:\n%s  %s\n", fn, class_string(code),
                fn, (detail && *detail) ? detail : "");
        fflush(stderr);
        exit(code);
    }
    return code;
}

int err_return(Comm* c, const char* fn, int code)
{
    if (code == MPI_SUCCESS) return code;
    if (c == nullptr) c = world();
    return err_return_h(c ? c->errhandler : MPI_ERRORS_ARE_FATAL, fn, code);
}

// MpiaCommValidateHandle
int v_comm(MPI_Comm c, Comm** out)
{
    *out = nullptr;
    if (c == MPI_COMM_NULL) { set_error("null communicator"); return MPI_ERR_COMM; }
    Comm* p = lookup_comm(c);
    if (!p) { set_error("invalid communicator 0x%x", c); return MPI_ERR_COMM; }
    *out = p;
    return MPI_SUCCESS;
}

// MpiaCommValidateIntracomm: an intercommunicator is MPI_ERR_COMM (**commnotintra)
int v_intracomm(MPI_Comm c, Comm** out)
{
    int rc = v_comm(c, out);
    if (rc == MPI_SUCCESS && (*out)->inter) {
        set_error("an intercommunicator is not valid here (**commnotintra)");
        rc = MPI_ERR_COMM;
    }
    return rc;
}

// MpiaDatatypeValidate (mpi_api.h:113-169), predefined datatypes only.
int v_dtype(const void* buf, long long count, MPI_Datatype dt)
{
    if (count == 0) return MPI_SUCCESS;
    if (count < 0) { set_error("negative count %lld", count); return MPI_ERR_COUNT; }
    if (dt == MPI_DATATYPE_NULL) { set_error("null datatype"); return MPI_ERR_TYPE; }
    if (!dtype_known(dt)) { set_error("invalid datatype 0x%x", dt); return MPI_ERR_TYPE; }
    if (buf == nullptr) { set_error("null buffer"); return MPI_ERR_BUFFER; }
    return MPI_SUCCESS;
}

// MpiaDatatypeValidate (mpi_api.h:113-164) with derived datatypes: the
// one-sided calls and MPI_Reduce_local (user ops) accept committed derived types.
int v_dtype_any(const void* buf, long long count, MPI_Datatype dt)
{
    if (count == 0) return MPI_SUCCESS;
    if (count < 0) { set_error("negative count %lld", count); return MPI_ERR_COUNT; }
    if (dt == MPI_DATATYPE_NULL) { set_error("null datatype"); return MPI_ERR_TYPE; }
    if (!dtype_is_derived(dt)) return v_dtype(buf, count, dt);
    Dtype* t;
    if (const int rc = v_committed_type(dt, &t)) return rc;
    if (buf == nullptr && t->true_lb == 0 && t->size > 0) { set_error("null buffer"); return MPI_ERR_BUFFER; }
    return MPI_SUCCESS;
}

// MpiaDatatypeValidateBuffer (mpi_api.h:190-212)
int v_buffer(MPI_Datatype dt, const void* buf, long long count)
{
    if (dtype_is_derived(dt)) {
        const Dtype* t = dtype_lookup(dt);
        if (buf == nullptr && count > 0 && t && t->true_lb == 0 && t->size > 0) {
            set_error("null buffer");
            return MPI_ERR_BUFFER;
        }
        return MPI_SUCCESS;
    }
    if (buf == nullptr && count > 0 && type_size(dt) > 0) {
        set_error("null buffer");
        return MPI_ERR_BUFFER;
    }
    return MPI_SUCCESS;
}

// MpiaOpValidateHandle (mpi_api.h:707-728)
int v_op_handle(MPI_Op op, OpRef* out)
{
    if (handle_kind(op) != OBJ_OP || handle_type(op) == HT_INVALID) {
        set_error("invalid MPI_Op 0x%x", op);
        return MPI_ERR_OP;
    }
    if (handle_type(op) == HT_BUILTIN) {
        int idx = op & 0xff;
        if (idx == kSumWideHandleIdx) idx = O_SUM_WIDE;      // MSX_SUM_WIDE (msx.h)
        else if (idx > O_NOOP) idx = O_NULL;                 // no other index is a builtin op
        if (idx < O_MAX || (op & 0x03ffff00)) {
            set_error("invalid builtin MPI_Op 0x%x", op);
            return MPI_ERR_OP;
        }
        out->opidx = idx;
        out->user_fn = nullptr;
        out->dev_fn = nullptr;
        out->dev_state = nullptr;
        out->dev_tree = nullptr;
        out->commutative = (idx != O_REPLACE && idx != O_NOOP);
        return MPI_SUCCESS;
    }
    std::lock_guard<std::mutex> g(g_op_mu);
    size_t idx = (size_t)(op & 0x03ffffff);
    if (handle_type(op) != HT_DIRECT || idx >= g_user_ops.size() || !g_user_ops[idx].live) {
        set_error("MPI_Op 0x%x does not name a live operation", op);
        return MPI_ERR_OP;
    }
    out->opidx = O_NULL;
    out->user_fn = g_user_ops[idx].fn;
    out->dev_fn = g_user_ops[idx].dev_fn;
    out->dev_state = g_user_ops[idx].dev_state;
    out->dev_tree = g_user_ops[idx].dev_tree;
    out->commutative = g_user_ops[idx].commute;
    return MPI_SUCCESS;
}

// Intercommunicator reductions are a frozen layer: no device user ops there.
int v_no_device_op_inter(const Comm* c, const OpRef& r)
{
    if (c->inter && r.dev_fn) {
        set_error("device user ops are not supported on intercommunicators");
        return MPI_ERR_OP;
    }
    if (c->inter && r.opidx == O_SUM_WIDE) {
        set_error("MSX_SUM_WIDE is not supported on intercommunicators");
        return MPI_ERR_OP;
    }
    return MPI_SUCCESS;
}

// MSX_SUM_WIDE is defined for one fused tree over raw contributions (msx.h).
// Calls whose steps exchange rounded partials (the scans) or combine into a
// remote target (one-sided) refuse it here, in the local argument checks:
// every rank fails alike, before any communication or device use.
int v_no_sum_wide(const OpRef& r, const char* what)
{
    if (r.opidx != O_SUM_WIDE) return MPI_SUCCESS;
    set_error("MSX_SUM_WIDE is not defined for %s", what);
    return MPI_ERR_OP;
}

// The op of the typed accumulate family (msx_api_acc.cpp): a valid handle, not
// MSX_SUM_WIDE (`reason` says why and what to use instead), and a builtin op.
int v_builtin_op(MPI_Op op, const char* entry, const char* reason, OpRef* out)
{
    const int rc = v_op_handle(op, out);
    if (rc != MPI_SUCCESS) return rc;
    if (out->opidx == O_SUM_WIDE) return v_no_sum_wide(*out, (std::string(entry) + " (" + reason + ")").c_str());
    if (out->opidx == O_NULL) { set_error("%s takes builtin ops only", entry); return MPI_ERR_OP; }
    return MPI_SUCCESS;
}

// MpiaOpValidate (mpi_api.h:731-775), rmaOp = false
int v_op(MPI_Op op, MPI_Datatype dt, OpRef* out)
{
    int rc = v_op_handle(op, out);
    if (rc != MPI_SUCCESS) return rc;
    if (out->opidx == O_REPLACE) { set_error("MPI_REPLACE not allowed"); return MPI_ERR_OP; }
    if (out->opidx == O_NOOP) { set_error("MPI_NO_OP not allowed"); return MPI_ERR_OP; }
    if (out->opidx != O_NULL) {
        rc = op_check_dtype(out->opidx, dt);
        if (rc != MPI_SUCCESS) {
            set_error("MPI_Op 0x%x (%s) is not defined for datatype 0x%x", op, op_name(out->opidx), dt);
            return rc;
        }
    }
    return MPI_SUCCESS;
}

// ---- the untraced init check, error return and communicator check (msx_api.h) ----
void api_require_init(const char* fn)
{
    if (!is_initialized() || is_finalized()) not_initialized_exit(fn);
}
int api_err_return(const char* fn, int code) { return err_return(nullptr, fn, code); }
int api_comm_valid(MPI_Comm comm)
{
    Comm* c;
    return v_comm(comm, &c);
}
}  // namespace msx

// ===========================================================================
// environment
// ===========================================================================
namespace {
int g_thread_level = MPI_THREAD_SINGLE;     // Mpi.ThreadLevel
std::thread::id g_main_thread;              // the thread that initialised MPI
}

MSX_EXPORT int MPI_Init(int* argc, char*** argv)
{
    (void)argc; (void)argv;
    if (is_initialized()) {
        set_error("MPI_Init called twice");
        return err_return(nullptr, "MPI_Init", MPI_ERR_OTHER);
    }
    int rc = world_init();
    if (rc != MPI_SUCCESS) {
        fprintf(stderr, "Fatal error in MPI_Init: %s\n", last_error());
        exit(rc);
    }
    g_thread_level = MPI_THREAD_SINGLE;       // mpi_env.cpp:167
    g_main_thread = std::this_thread::get_id();
    return MPI_SUCCESS;
}

MSX_EXPORT int MPI_Init_thread(int* argc, char*** argv, int required, int* provided)
{
    int rc = MPI_Init(argc, argv);
    // Kernels are reentrant; the host staging path and bootstrap are locked
    // (mid/env.cpp:1071-1078 grants up to MULTIPLE).
    const int level = required > MPI_THREAD_MULTIPLE ? MPI_THREAD_MULTIPLE : required;
    if (rc == MPI_SUCCESS) g_thread_level = level;
    if (provided) *provided = level;
    return rc;
}

MSX_EXPORT int MPI_Finalize(void)
{
    MSX_REQUIRE_INIT("MPI_Finalize");
    return world_finalize();
}

MSX_EXPORT int MPI_Initialized(int* flag)
{
    if (!flag) return MPI_ERR_ARG;
    *flag = is_initialized() ? 1 : 0;
    return MPI_SUCCESS;
}

MSX_EXPORT int MPI_Finalized(int* flag)
{
    if (!flag) return MPI_ERR_ARG;
    *flag = is_finalized() ? 1 : 0;
    return MPI_SUCCESS;
}

MSX_EXPORT int MPI_Abort(MPI_Comm comm, int errorcode)
{
    (void)comm;
    fprintf(stderr, "MPI_Abort called with error code %d\n", errorcode);
    fflush(stderr);
    exit(errorcode);
}

MSX_EXPORT double MPI_Wtime(void)
{
    using namespace std::chrono;
    return duration<double>(steady_clock::now().time_since_epoch()).count();
}

// the resolution of MPI_Wtime's clock (mpi_env.cpp:767)
MSX_EXPORT double MPI_Wtick(void)
{
    using namespace std::chrono;
    return duration<double>(steady_clock::duration(1)).count();
}

// mpi_env.cpp:575-610: the level MPI_Init / MPI_Init_thread provided
MSX_EXPORT int MPI_Query_thread(int* provided)
{
    MSX_REQUIRE_INIT("MPI_Query_thread");
    if (!provided) { set_error("**nullptr provided"); return err_return(nullptr, "MPI_Query_thread", MPI_ERR_ARG); }
    *provided = g_thread_level;
    return MPI_SUCCESS;
}

// mpi_env.cpp:463-500: is the caller the thread that initialised MPI
MSX_EXPORT int MPI_Is_thread_main(int* flag)
{
    MSX_REQUIRE_INIT("MPI_Is_thread_main");
    if (!flag) { set_error("**nullptr flag"); return err_return(nullptr, "MPI_Is_thread_main", MPI_ERR_ARG); }
    *flag = std::this_thread::get_id() == g_main_thread ? 1 : 0;
    return MPI_SUCCESS;
}

// mpi_env.cpp:630-680; callable before MPI_Init
MSX_EXPORT int MPI_Get_version(int* version, int* subversion)
{
    if (!version || !subversion) {
        set_error("**nullptr %s", version ? "subversion" : "version");
        return is_initialized() ? err_return(nullptr, "MPI_Get_version", MPI_ERR_ARG) : MPI_ERR_ARG;
    }
    *version = MPI_VERSION;
    *subversion = MPI_SUBVERSION;
    return MPI_SUCCESS;
}

// mpi_env.cpp:1095-1140 (MPID_Get_processor_name: the host name)
MSX_EXPORT int MPI_Get_processor_name(char* name, int* resultlen)
{
    MSX_REQUIRE_INIT("MPI_Get_processor_name");
    if (!name || !resultlen) {
        set_error("**nullptr %s", name ? "resultlen" : "name");
        return err_return(nullptr, "MPI_Get_processor_name", MPI_ERR_ARG);
    }
    char host[MPI_MAX_PROCESSOR_NAME] = {0};
    if (gethostname(host, sizeof(host) - 1) != 0) snprintf(host, sizeof(host), "localhost");
    const size_t n = strnlen(host, MPI_MAX_PROCESSOR_NAME - 1);
    memcpy(name, host, n);
    name[n] = 0;
    *resultlen = (int)n;
    return MPI_SUCCESS;
}

MSX_EXPORT int MPI_Comm_rank(MPI_Comm comm, int* rank)
{
    MSX_REQUIRE_INIT("MPI_Comm_rank");
    Comm* c;
    int rc = v_comm(comm, &c);
    if (rc == MPI_SUCCESS && !rank) { set_error("null rank"); rc = MPI_ERR_ARG; }
    if (rc != MPI_SUCCESS) return err_return(nullptr, "MPI_Comm_rank", rc);
    *rank = c->rank;
    return MPI_SUCCESS;
}

MSX_EXPORT int MPI_Comm_size(MPI_Comm comm, int* size)
{
    MSX_REQUIRE_INIT("MPI_Comm_size");
    Comm* c;
    int rc = v_comm(comm, &c);
    if (rc == MPI_SUCCESS && !size) { set_error("null size"); rc = MPI_ERR_ARG; }
    if (rc != MPI_SUCCESS) return err_return(nullptr, "MPI_Comm_size", rc);
    *size = c->size;
    return MPI_SUCCESS;
}

// ---- derived communicators (api/mpi_comm.cpp: MPI_Comm_split / dup / free) ------
// Reductions on sub-communicators need them: each group gets its own
// transport (hub, shared-memory barrier, engine windows) and runs the same
// reference-order schedules over its own ranks.
MSX_EXPORT int MPI_Comm_split(MPI_Comm comm, int color, int key, MPI_Comm* newcomm)
{
    MSX_REQUIRE_INIT("MPI_Comm_split");
    Comm* c;
    int rc = v_intracomm(comm, &c);     // intercommunicator splits are not supported
    if (rc == MPI_SUCCESS && !newcomm) { set_error("null newcomm"); rc = MPI_ERR_ARG; }
    if (rc == MPI_SUCCESS && color < 0 && color != MPI_UNDEFINED) {
        set_error("color %d is negative and not MPI_UNDEFINED", color);
        rc = MPI_ERR_ARG;
    }
    Comm* n = nullptr;
    if (rc == MPI_SUCCESS) rc = engine_comm_split(c, color, key, &n);
    if (rc != MPI_SUCCESS) return err_return(c, "MPI_Comm_split", rc);
    *newcomm = n ? comm_register(n) : MPI_COMM_NULL;
    return MPI_SUCCESS;
}

MSX_EXPORT int MPI_Comm_dup(MPI_Comm comm, MPI_Comm* newcomm)
{
    MSX_REQUIRE_INIT("MPI_Comm_dup");
    Comm* c;
    int rc = v_comm(comm, &c);
    if (rc == MPI_SUCCESS && !newcomm) { set_error("null newcomm"); rc = MPI_ERR_ARG; }
    Comm* n = nullptr;
    if (rc == MPI_SUCCESS && c->inter) rc = engine_intercomm_dup(c, &n);
    else if (rc == MPI_SUCCESS) rc = engine_comm_split(c, 0, c->rank, &n);   // same group, same order
    if (rc != MPI_SUCCESS) return err_return(c, "MPI_Comm_dup", rc);
    *newcomm = comm_register(n);
    return MPI_SUCCESS;
}

// api/mpi_comm.cpp:184-248, MPIR_Comm_create_intra (mpid/comm.cpp:1027-1128):
// collective over `comm`; members get a communicator ranked in group order,
// the others MPI_COMM_NULL.  A group member outside `comm` is MPI_ERR_GROUP
// (**groupnotincomm, comm.cpp:977) on the members, after the collective step
// every process takes (here the split, there the context id).
MSX_EXPORT int MPI_Comm_create(MPI_Comm comm, MPI_Group group, MPI_Comm* newcomm)
{
    MSX_REQUIRE_INIT("MPI_Comm_create");
    Comm* c;
    int rc = v_intracomm(comm, &c);     // MPIR_Comm_create_inter is not supported
    if (rc != MPI_SUCCESS) return err_return(nullptr, "MPI_Comm_create", rc);
    std::vector<int> members;
    rc = group_members(group, &members);
    if (rc == MPI_SUCCESS && !newcomm) { set_error("null newcomm"); rc = MPI_ERR_ARG; }
    if (rc != MPI_SUCCESS) return err_return(c, "MPI_Comm_create", rc);
    const int me = c->lpid.empty() ? c->rank : c->lpid[(size_t)c->rank];
    int grank = MPI_UNDEFINED;
    bool valid = true;
    for (size_t i = 0; i < members.size(); ++i) {
        if (members[i] == me) grank = (int)i;
        if (std::find(c->lpid.begin(), c->lpid.end(), members[i]) == c->lpid.end()) valid = false;
    }
    Comm* n = nullptr;
    rc = engine_comm_split(c, grank != MPI_UNDEFINED && valid ? 0 : MPI_UNDEFINED, grank, &n);
    if (rc == MPI_SUCCESS && grank != MPI_UNDEFINED && !valid) {
        set_error("**groupnotincomm: a group member is not in the communicator");
        rc = MPI_ERR_GROUP;
    }
    if (rc != MPI_SUCCESS) return err_return(c, "MPI_Comm_create", rc);
    *newcomm = n ? comm_register(n) : MPI_COMM_NULL;
    return MPI_SUCCESS;
}

// api/mpi_comm.cpp:51-157 (intracommunicators): IDENT for the same handle,
// else the groups' relation with IDENT promoted to CONGRUENT
MSX_EXPORT int MPI_Comm_compare(MPI_Comm comm1, MPI_Comm comm2, int* result)
{
    MSX_REQUIRE_INIT("MPI_Comm_compare");
    Comm *c1, *c2 = nullptr;
    int rc = v_comm(comm1, &c1);
    if (rc == MPI_SUCCESS) rc = v_comm(comm2, &c2);
    if (rc == MPI_SUCCESS && !result) { set_error("**nullptr result"); rc = MPI_ERR_ARG; }
    if (rc != MPI_SUCCESS) return err_return(nullptr, "MPI_Comm_compare", rc);
    auto rel = [](const std::vector<int>& x, const std::vector<int>& y) {
        if (x == y) return MPI_IDENT;
        std::vector<int> a = x, b = y;
        std::sort(a.begin(), a.end());
        std::sort(b.begin(), b.end());
        return a == b ? MPI_SIMILAR : MPI_UNEQUAL;
    };
    if (c1->inter != c2->inter) {
        *result = MPI_UNEQUAL;
    } else if (comm1 == comm2) {
        *result = MPI_IDENT;
    } else {
        // groups (and, for intercommunicators, remote groups too: the weaker
        // relation of the two); identical groups under another handle are
        // congruent
        int r = rel(c1->lpid, c2->lpid);
        if (c1->inter) r = std::max(r, rel(c1->remote_lpid, c2->remote_lpid));
        *result = r == MPI_IDENT ? MPI_CONGRUENT : r;
    }
    return MPI_SUCCESS;
}

// api/mpi_comm.cpp:1386-1420
MSX_EXPORT int MPI_Comm_test_inter(MPI_Comm comm, int* flag)
{
    MSX_REQUIRE_INIT("MPI_Comm_test_inter");
    Comm* c;
    int rc = v_comm(comm, &c);
    if (rc == MPI_SUCCESS && !flag) { set_error("**nullptr flag"); rc = MPI_ERR_ARG; }
    if (rc != MPI_SUCCESS) return err_return(nullptr, "MPI_Comm_test_inter", rc);
    *flag = c->inter ? 1 : 0;
    return MPI_SUCCESS;
}

// ---- intercommunicators (api/mpi_comm.cpp:835-960, 1482-1830) ------------------
MSX_EXPORT int MPI_Comm_remote_size(MPI_Comm comm, int* size)
{
    MSX_REQUIRE_INIT("MPI_Comm_remote_size");
    Comm* c;
    int rc = v_comm(comm, &c);
    if (rc == MPI_SUCCESS && !c->inter) { set_error("**commnotinter"); rc = MPI_ERR_COMM; }
    if (rc == MPI_SUCCESS && !size) { set_error("**nullptr size"); rc = MPI_ERR_ARG; }
    if (rc != MPI_SUCCESS) return err_return(c, "MPI_Comm_remote_size", rc);
    *size = (int)c->remote_lpid.size();
    return MPI_SUCCESS;
}

MSX_EXPORT int MPI_Comm_remote_group(MPI_Comm comm, MPI_Group* group)
{
    MSX_REQUIRE_INIT("MPI_Comm_remote_group");
    Comm* c;
    int rc = v_comm(comm, &c);
    if (rc == MPI_SUCCESS && !c->inter) { set_error("**commnotinter"); rc = MPI_ERR_COMM; }
    if (rc == MPI_SUCCESS && !group) { set_error("**nullptr group"); rc = MPI_ERR_ARG; }
    if (rc == MPI_SUCCESS) rc = group_create(c->remote_lpid, group);
    return err_return(c, "MPI_Comm_remote_group", rc);
}

// The leaders exchange their groups over the world mailbox; both groups then
// join one bootstrap hub (the low group's rank 0), which carries the windows
// and flags of the transfers between the groups.
MSX_EXPORT int MPI_Intercomm_create(MPI_Comm local_comm, int local_leader, MPI_Comm peer_comm, int remote_leader,
                                    int tag, MPI_Comm* newintercomm)
{
    MSX_REQUIRE_INIT("MPI_Intercomm_create");
    Comm *c, *peer = nullptr;
    int rc = v_intracomm(local_comm, &c);
    if (rc == MPI_SUCCESS && (local_leader < 0 || local_leader >= c->size)) {
        set_error("**ranklocal %d %d", local_leader, c->size);
        rc = MPI_ERR_RANK;
    }
    if (rc == MPI_SUCCESS && c->rank == local_leader) {
        rc = v_comm(peer_comm, &peer);
        if (rc == MPI_SUCCESS && peer->inter) {
            set_error("an intercommunicator as peer_comm is not supported");
            rc = MPI_ERR_COMM;
        }
        if (rc == MPI_SUCCESS && (remote_leader < 0 || remote_leader >= peer->size)) {
            set_error("**rankremote %d %d", remote_leader, peer->size);
            rc = MPI_ERR_RANK;
        }
        if (rc == MPI_SUCCESS && peer->rank == remote_leader) {
            set_error("**ranksdistinct");
            rc = MPI_ERR_RANK;
        }
    }
    if (rc == MPI_SUCCESS && !newintercomm) { set_error("**nullptr newintercomm"); rc = MPI_ERR_ARG; }
    Comm* n = nullptr;
    if (rc == MPI_SUCCESS) rc = engine_intercomm_create(c, local_leader, peer, remote_leader, tag, &n);
    if (rc != MPI_SUCCESS) return err_return(c, "MPI_Intercomm_create", rc);
    *newintercomm = comm_register(n);
    return MPI_SUCCESS;
}

MSX_EXPORT int MPI_Intercomm_merge(MPI_Comm intercomm, int high, MPI_Comm* newintracomm)
{
    MSX_REQUIRE_INIT("MPI_Intercomm_merge");
    Comm* c;
    int rc = v_comm(intercomm, &c);
    if (rc == MPI_SUCCESS && !c->inter) { set_error("**commnotinter"); rc = MPI_ERR_COMM; }
    if (rc == MPI_SUCCESS && !newintracomm) { set_error("**nullptr newintracomm"); rc = MPI_ERR_ARG; }
    Comm* n = nullptr;
    if (rc == MPI_SUCCESS) rc = engine_intercomm_merge(c, high, &n);
    if (rc != MPI_SUCCESS) return err_return(c, "MPI_Intercomm_merge", rc);
    *newintracomm = comm_register(n);
    return MPI_SUCCESS;
}

MSX_EXPORT int MPI_Comm_free(MPI_Comm* comm)
{
    MSX_REQUIRE_INIT("MPI_Comm_free");
    if (!comm) { set_error("null comm"); return err_return(nullptr, "MPI_Comm_free", MPI_ERR_ARG); }
    Comm* c;
    int rc = v_comm(*comm, &c);
    if (rc != MPI_SUCCESS) return err_return(nullptr, "MPI_Comm_free", rc);
    if (c == lookup_comm(MPI_COMM_WORLD) || c == lookup_comm(MPI_COMM_SELF)) {
        set_error("a predefined communicator cannot be freed (**commperm)");
        return err_return(c, "MPI_Comm_free", MPI_ERR_COMM);
    }
    rc = engine_comm_free(c);
    comm_unregister(c);
    delete c;
    *comm = MPI_COMM_NULL;
    return rc == MPI_SUCCESS ? MPI_SUCCESS : err_return(nullptr, "MPI_Comm_free", rc);
}

MSX_EXPORT int MPI_Barrier(MPI_Comm comm)
{
    MSX_REQUIRE_INIT("MPI_Barrier");
    Comm* c;
    int rc = v_comm(comm, &c);
    if (rc == MPI_SUCCESS) rc = coll_barrier(c->inter ? c->uni : c);   // intercomm: both groups
    return err_return(c, "MPI_Barrier", rc);
}

MSX_EXPORT int MPI_Comm_set_errhandler(MPI_Comm comm, MPI_Errhandler eh)
{
    MSX_REQUIRE_INIT("MPI_Comm_set_errhandler");
    Comm* c;
    int rc = v_comm(comm, &c);
    if (rc == MPI_SUCCESS && eh != MPI_ERRORS_ARE_FATAL && eh != MPI_ERRORS_RETURN) {
        set_error("unsupported errhandler 0x%x", eh);
        rc = MPI_ERR_ARG;
    }
    if (rc != MPI_SUCCESS) return err_return(c, "MPI_Comm_set_errhandler", rc);
    c->errhandler = eh;
    return MPI_SUCCESS;
}

MSX_EXPORT int MPI_Comm_get_errhandler(MPI_Comm comm, MPI_Errhandler* eh)
{
    MSX_REQUIRE_INIT("MPI_Comm_get_errhandler");
    Comm* c;
    int rc = v_comm(comm, &c);
    if (rc == MPI_SUCCESS && !eh) rc = MPI_ERR_ARG;
    if (rc != MPI_SUCCESS) return err_return(c, "MPI_Comm_get_errhandler", rc);
    *eh = c->errhandler;
    return MPI_SUCCESS;
}

MSX_EXPORT int MPI_Error_class(int errorcode, int* errorclass)
{
    if (!errorclass) return MPI_ERR_ARG;
    // This library returns error classes as codes.
    *errorclass = errorcode & 0x7f;
    return MPI_SUCCESS;
}

MSX_EXPORT int MPI_Error_string(int errorcode, char* str, int* len)
{
    if (!str || !len) return MPI_ERR_ARG;
    int n = snprintf(str, MPI_MAX_ERROR_STRING, "%s", class_string(errorcode & 0x7f));
    *len = n < MPI_MAX_ERROR_STRING ? n : MPI_MAX_ERROR_STRING - 1;
    return MPI_SUCCESS;
}

// ===========================================================================
// operations (api/mpi_op.cpp:48-260)
// ===========================================================================
MSX_EXPORT int MPI_Op_create(MPI_User_function* user_fn, int commute, MPI_Op* op)
{
    MSX_REQUIRE_INIT("MPI_Op_create");
    int rc = MPI_SUCCESS;
    if (user_fn == nullptr) { set_error("null user_fn"); rc = MPI_ERR_ARG; }
    else if (op == nullptr) { set_error("null op"); rc = MPI_ERR_ARG; }
    if (rc != MPI_SUCCESS) return err_return(nullptr, "MPI_Op_create", rc);
    *op = op_pool_add(UserOp{user_fn, commute != 0, true, nullptr, nullptr, nullptr});
    return MPI_SUCCESS;
}

MSX_EXPORT int msx_op_create_device(MSX_Device_function* fn, int commute, void* state, MPI_Op* op)
{
    MSX_REQUIRE_INIT("msx_op_create_device");
    return device_op_create(fn, nullptr, commute, state, op);
}

// The same op with a fused tree function beside the pairwise one (msx.h): the
// reduction collectives call it once per evaluating rank (msx_devop.cpp).
MSX_EXPORT int msx_op_create_device_tree(MSX_Device_function* fn, MSX_Device_tree_function* tree_fn, int commute,
                                         void* state, MPI_Op* op)
{
    MSX_REQUIRE_INIT("msx_op_create_device_tree");
    return device_op_create(fn, tree_fn, commute, state, op);
}

MSX_EXPORT int msx_op_has_device_tree(MPI_Op op)
{
    OpRef r;
    if (v_op_handle(op, &r) != MPI_SUCCESS) return -1;
    return r.dev_tree ? 1 : 0;
}

MSX_EXPORT int msx_op_is_device(MPI_Op op)
{
    OpRef r;
    if (v_op_handle(op, &r) != MPI_SUCCESS) return -1;
    return r.dev_fn ? 1 : 0;
}

MSX_EXPORT int MPI_Op_free(MPI_Op* op)
{
    MSX_REQUIRE_INIT("MPI_Op_free");
    int rc = MPI_SUCCESS;
    OpRef r;
    if (op == nullptr) { set_error("null op"); rc = MPI_ERR_ARG; }
    else rc = v_op_handle(*op, &r);
    if (rc == MPI_SUCCESS && r.opidx != O_NULL) {
        set_error("cannot free permanent MPI_Op");   // "**permop" mpi_op.cpp:169-173
        rc = MPI_ERR_OP;
    }
    if (rc != MPI_SUCCESS) return err_return(nullptr, "MPI_Op_free", rc);
    std::lock_guard<std::mutex> g(g_op_mu);
    g_user_ops[(size_t)(*op & 0x03ffffff)].live = false;
    *op = MPI_OP_NULL;
    return MPI_SUCCESS;
}

MSX_EXPORT int MPI_Op_commutative(MPI_Op op, int* commute)
{
    MSX_REQUIRE_INIT("MPI_Op_commutative");
    OpRef r;
    int rc = v_op_handle(op, &r);
    if (rc == MPI_SUCCESS && commute == nullptr) { set_error("null commute"); rc = MPI_ERR_ARG; }
    if (rc != MPI_SUCCESS) return err_return(nullptr, "MPI_Op_commutative", rc);
    *commute = r.commutative ? 1 : 0;
    return MPI_SUCCESS;
}


// ---- PMPI_ profiling aliases (dll/msmpi.def) --------------------------------
MSX_ALIAS(MPI_Comm_create) int PMPI_Comm_create(MPI_Comm, MPI_Group, MPI_Comm*);
MSX_ALIAS(MPI_Comm_compare) int PMPI_Comm_compare(MPI_Comm, MPI_Comm, int*);
MSX_ALIAS(MPI_Intercomm_create) int PMPI_Intercomm_create(MPI_Comm, int, MPI_Comm, int, int, MPI_Comm*);
MSX_ALIAS(MPI_Intercomm_merge) int PMPI_Intercomm_merge(MPI_Comm, int, MPI_Comm*);
MSX_ALIAS(MPI_Op_create) int PMPI_Op_create(MPI_User_function*, int, MPI_Op*);
MSX_ALIAS(MPI_Op_free) int PMPI_Op_free(MPI_Op*);
MSX_ALIAS(MPI_Op_commutative) int PMPI_Op_commutative(MPI_Op, int*);
