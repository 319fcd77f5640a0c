// msx_api.h — what the C entry-point units share: the export macros, the
// entry check, the error return and the argument validators.
//
// Internal to the entry-point units (msx_api*.cpp, msx_api_acc.cpp included,
// msx_dtype_api.cpp, msx_group.cpp); never included by a .hip unit or by the engine units.  Each
// function has one owner unit, named beside it.
#pragma once

#include "../../include/msx.h"
#include "msx_comm.h"
#include "msx_runtime.h"
#include "msx_types.h"

#define MSX_EXPORT extern "C" __attribute__((visibility("default")))
// PMPI_ profiling aliases (dll/msmpi.def).  An alias needs its target in the
// same translation unit: each unit lists the aliases of its own functions.
#define MSX_ALIAS(name) extern "C" __attribute__((visibility("default"), alias(#name)))

// Entry of every MPI call: MpiaIsInitializedOrExit, then an API range that
// spans the rest of the call (ApiRange, msx_runtime.h).
#define MSX_REQUIRE_INIT(fn)                                                  \
    if (!is_initialized() || is_finalized()) not_initialized_exit(fn);        \
    ApiRange msx_api_range_(fn)

namespace msx {

// ---- msx_api.cpp -------------------------------------------------------------
// MpiaIsInitializedOrExit -> MPIR_Err_preOrPostInit (api/mpi_api.h:27)
void not_initialized_exit(const char* fn);
// MPIR_Err_return_comm (mpid/error.cpp:85-134): the handler of `c`, of
// MPI_COMM_WORLD when c is null; ERRORS_ARE_FATAL aborts the job.
int err_return_h(MPI_Errhandler h, const char* fn, int code);
int err_return(Comm* c, const char* fn, int code);

int v_comm(MPI_Comm c, Comm** out);           // MpiaCommValidateHandle
int v_intracomm(MPI_Comm c, Comm** out);      // MpiaCommValidateIntracomm
// MpiaDatatypeValidate (mpi_api.h:113-169): predefined datatypes only / with
// committed derived datatypes
int v_dtype(const void* buf, long long count, MPI_Datatype dt);
int v_dtype_any(const void* buf, long long count, MPI_Datatype dt);
int v_buffer(MPI_Datatype dt, const void* buf, long long count);   // MpiaDatatypeValidateBuffer
// MpiaOpValidateHandle / MpiaOpValidate (rmaOp = false); they read the op pool
int v_op_handle(MPI_Op op, OpRef* out);
int v_op(MPI_Op op, MPI_Datatype dt, OpRef* out);
int v_no_device_op_inter(const Comm* c, const OpRef& r);
int v_no_sum_wide(const OpRef& r, const char* what);
// v_op_handle, v_no_sum_wide(r, "<entry> (<reason>)"), "<entry> takes builtin ops only"
int v_builtin_op(MPI_Op op, const char* entry, const char* reason, OpRef* out);

// ---- msx_dtype_api.cpp -------------------------------------------------------
struct Dtype;
// MpiaDatatypeValidateHandle + MpiaDatatypeValidateCommitted (mpi_api.h:53-111)
int v_committed_type(MPI_Datatype h, Dtype** out);

// The entry points of msx_dtype_api.cpp and msx_group.cpp are not traced (no
// device work of their own except MPI_Pack / MPI_Unpack, which open their own
// range): they take the init check without the ApiRange.
void api_require_init(const char* fn);              // MpiaIsInitializedOrExit
int api_err_return(const char* fn, int code);       // MPIR_Err_return_comm(NULL, ...)
int api_comm_valid(MPI_Comm comm);                   // MpiaCommValidateHandle

}  // namespace msx
