/*
 * msx.h — device-side C ABI of the MI355X MS-MPI reduction path.
 *
 * Plain C, no HIP/torch types: streams are passed as `void*` (a hipStream_t,
 * NULL = the HIP null stream, as with any HIP API).
 *
 * Each entry point names the reference interface it replaces:
 *
 *   msx_reduce_local_dev  <- MPID_Uop_call(op, in, inout, &len, &dt)
 *                            (src/mpi/msmpi/include/op.h:171-174) reaching
 *                            MPIR_Op_<op>(void*, void*, int*, MPI_Datatype*)
 *                            (src/mpi/msmpi/mpid/op.cpp:703-1795), with the
 *                            MPI_Reduce_local argument checks
 *                            (src/mpi/msmpi/api/mpi_reduce.cpp:304-385);
 *                            64-bit count, stream-ordered, device pointers.
 *   msx_op_check          <- MPIR_Op_check_dtype_table[op%16-1](dt)
 *                            (op.cpp:653-672, api/mpi_api.h:765)
 *   msx_pack_dev /        <- MPID_Segment_pack / MPID_Segment_unpack over a
 *   msx_unpack_dev           committed datatype (src/mpi/msmpi/mpid/segment.cpp,
 *                            called by MPI_Pack/MPI_Unpack, api/mpi_pack.cpp:41-660);
 *                            64-bit count, stream-ordered, device pointers.
 *   msx_accumulate_dev    <- MPID_Uop_call(origin, target) over a derived target
 *                            (win.cpp:1435, packethandling.cpp:2969-3004) and
 *                            the two-datatype MPIR_Localcopy (mpid/pt2pt.cpp:
 *                            770-948), with a type map on BOTH sides.
 *   msx_accumulate_widen_dev <- not in the reference: the same MPID_Uop_call on
 *                            MPI_FLOAT with the origin held as 16-bit floats,
 *                            widened exactly on the way in.
 *   msx_fetch_and_op_dev /<- the target side of MPI_Fetch_and_op /
 *   msx_get_accumulate_dev   MPI_Get_accumulate (win.cpp:1804,
 *                            Handle_MPIDI_CH3_PKT_GET_ACCUMULATE,
 *                            packethandling.cpp:2121): the old target value
 *                            into the result, then MPID_Uop_call(origin, target).
 *   msx_reduce_tree_dev   <- the per-step MPID_Uop_call chain of the
 *                            recursive-halving/doubling schedules
 *                            (src/mpi/msmpi/mpid/reduce.cpp:3899-3989,
 *                            1088-1175) fused into one pass over p inputs.
 *
 * All functions return an MPI error class (MPI_SUCCESS = 0).  Extensions do
 * not invoke the MPI error handler; msx_last_error() describes the failure.
 */
#ifndef MSX_H_INCLUDED
#define MSX_H_INCLUDED

#include <stdint.h>
#include "mpi.h"

/* 16-bit floating-point datatypes (extensions: MS-MPI predefines none, and
 * mpi.h keeps MPI_REAL2 == MPI_DATATYPE_NULL).  Builtin-datatype handles in
 * the 0x4c00SSII layout with size byte 02 and indices clear of mpi.h's (which
 * end at 0x3d).  MSX_FLOAT16 is IEEE binary16, MSX_BFLOAT16 is bfloat16.
 * Legal with MPI_MAX, MPI_MIN, MPI_SUM and MPI_PROD (every other builtin op:
 * MPI_ERR_OP), with MPI_REPLACE / MPI_NO_OP in accumulates, with user ops, and
 * as the base of any derived datatype.  SUM / PROD widen both operands exactly
 * to fp32, do one IEEE fp32 operation and round the result to nearest-even
 * (subnormals kept, overflow to inf); a NaN result follows the x86 rule of the
 * fp32 path in the 16-bit format.  MAX / MIN return the chosen operand's bits
 * (inout > in ? inout : in on the widened values).  Trees and collectives round
 * at every combine. */
#define MSX_FLOAT16         ((MPI_Datatype)0x4c000250)
#define MSX_BFLOAT16        ((MPI_Datatype)0x4c000251)

/* MSX_SUM_WIDE: the fp32-accumulated tree sum of MSX_FLOAT16 / MSX_BFLOAT16
 * (an extension: MPI_SUM on these types is defined per combine and rounds at
 * every node).  A builtin-op handle in the 0x580000II layout with an index
 * clear of mpi.h's (0x01 .. 0x0e); 0x50 mirrors the datatypes' choice.
 *
 * Definition, with w(x) and n(r) as above:
 *   node   r = inout + in on widened values: one IEEE fp32 add, the left
 *          operand in the `inout` role, subnormals kept -- the library's fp32
 *          MPI_SUM combine.  A NaN r follows the x86 rule in fp32: inout's
 *          bits | 0x00400000 if inout is a NaN, else in's bits | 0x00400000,
 *          else 0xFFC00000.  (A 16-bit NaN widens with its sign and payload.)
 *   tree   a fused evaluation is ONE tree of msx_reduce_tree_spec_dev's shape
 *          (leaf pairs, balanced tree with absent leaves, or chain): the leaves
 *          are widened, every node is computed in fp32 in the reference's
 *          association, nothing is rounded in between;
 *   root   n(root) is stored; for a NaN root the truncation: sign, all-ones
 *          exponent, the top 10 (fp16) / 7 (bf16) mantissa bits.  A 16-bit NaN
 *          comes back with its payload and the format's quiet bit, the default
 *          NaN as 0xFE00 / 0xFFC0, and a one-source tree returns its source's
 *          bits unchanged (signalling NaNs included).
 * Over two sources the result equals MPI_SUM's on the same type, bit for bit.
 *
 * Legal with MSX_FLOAT16 and MSX_BFLOAT16 only (any other datatype:
 * MPI_ERR_OP); commutative; MPI_Op_free refuses it; msx_op_table returns NULL
 * (the reference's table index op % 16 - 1 cannot name it).
 * Accepted: msx_reduce_tree_dev / _spec_dev / _done_dev; MPI_Allreduce,
 * MPI_Reduce, MPI_Reduce_scatter[_block] and their non-blocking forms (each
 * rank's result is one fused tree over the gathered contributions);
 * MPI_Reduce_local, msx_reduce_local_dev, msx_reduce_local_batch_dev and
 * msx_reduce_local_multi (one combine: MPI_SUM's bytes).
 * Refused with MPI_ERR_OP in the local argument checks, before any
 * communication: MPI_Scan / MPI_Exscan / MPI_Iscan / MPI_Iexscan (their steps
 * exchange rounded partials, so there is no fused evaluation), every one-sided
 * call, and reductions on intercommunicators. */
#define MSX_SUM_WIDE        ((MPI_Op)0x58000050)

#ifdef __cplusplus
extern "C" {
#endif

/* library identity */
const char* msx_version(void);
/* number of visible GPUs (0 on a host without one); never aborts */
int msx_device_count(void);
/* data plane of the collective engine for MPI_COMM_WORLD: "rccl" (RCCL
 * send/recv over xGMI, MSX_TRANSPORT=rccl and one GPU per rank), "ipc" (IPC
 * windows + remote writes) or "self" (one rank) */
const char* msx_engine_transport(void);
/* 1 when two or more ranks of MPI_COMM_WORLD run on one GPU (their PCI bus ids
 * agree), 0 when every rank has its own GPU, -1 before MPI_Init; the same on
 * every rank.  Link fractions (xGMI) mean nothing when it is 1. */
int msx_engine_gpu_shared(void);
/* phase timers of the window allreduce since the last reset (seconds):
 * out[0] stage+scatter, [1] collect wait + barrier A, [2] reduce + push,
 * [3] barrier B, [4] final collect, [5] chunks, [6] calls, [7] calls that
 * took the GPU-flag Rabenseifner schedules (two-step allreduce / reduce,
 * flag reduce_scatter); returns 8 */
int msx_engine_stats(double* out, int n, int reset);
/* link roofline probe over MPI_COMM_WORLD (collective): every rank writes
 * bytes_per_peer (capped at the window sub-slot) into each peer's window at
 * once, reps timed repetitions; *seconds = median time of one all-peer write
 * of *bytes_used per peer.  Per-GPU outbound bandwidth =
 * (size-1) * *bytes_used / *seconds. */
int msx_peer_write_bandwidth(int64_t bytes_per_peer, int reps, double* seconds, int64_t* bytes_used);
/* text of the last error raised on the calling thread ("" if none) */
const char* msx_last_error(void);

/* (op, datatype) legality exactly as the reference's check tables */
int msx_op_check(MPI_Op op, MPI_Datatype datatype);
/* element size in bytes of a predefined datatype (-1 if unknown) */
int msx_type_size(MPI_Datatype datatype);

/* The builtin op table, MPIR_Op_table (src/mpi/msmpi/mpid/op.cpp:618-622),
 * entries MPIR_Op_<op> (op.cpp:703-1923): the MPI_User_function shape that
 * MPID_Uop_call (include/op.h:171-174), the NBC reduce tasks (tasks.cpp:667,
 * 680), RMA accumulate (win.cpp:1435) and the Fortran proxy (mpif.cpp:963-976)
 * call.  Blocking: `inout` holds the result on return; operands may be device
 * memory (the gfx950 kernels run on it) or host memory (offloaded like
 * MPI_Reduce_local).  *len <= 0 does nothing.  An unsupported (op, datatype)
 * pair leaves inout untouched and sets the calling thread's op_errno to
 * MPI_ERR_OP (op.cpp:1791); a GPU failure also lands there.
 * msx_op_table(op) returns the entry of MPI_MAX .. MPI_NO_OP (NULL for any
 * other handle). */
void msx_op_max(void* in, void* inout, int* len, MPI_Datatype* dt);
void msx_op_min(void* in, void* inout, int* len, MPI_Datatype* dt);
void msx_op_sum(void* in, void* inout, int* len, MPI_Datatype* dt);
void msx_op_prod(void* in, void* inout, int* len, MPI_Datatype* dt);
void msx_op_land(void* in, void* inout, int* len, MPI_Datatype* dt);
void msx_op_band(void* in, void* inout, int* len, MPI_Datatype* dt);
void msx_op_lor(void* in, void* inout, int* len, MPI_Datatype* dt);
void msx_op_bor(void* in, void* inout, int* len, MPI_Datatype* dt);
void msx_op_lxor(void* in, void* inout, int* len, MPI_Datatype* dt);
void msx_op_bxor(void* in, void* inout, int* len, MPI_Datatype* dt);
void msx_op_minloc(void* in, void* inout, int* len, MPI_Datatype* dt);
void msx_op_maxloc(void* in, void* inout, int* len, MPI_Datatype* dt);
void msx_op_replace(void* in, void* inout, int* len, MPI_Datatype* dt);   /* MPIR_Op_replace op.cpp:1886 */
void msx_op_noop(void* in, void* inout, int* len, MPI_Datatype* dt);      /* MPIR_Op_noop op.cpp:1906 */
MPI_User_function* msx_op_table(MPI_Op op);
/* 1 when both operands are device memory (HBM, managed or IPC-mapped), else 0
 * (host memory, NULL, or no GPU).  The routing test of the table binding
 * (INTEGRATION.md section 2): device operands go to msx_op_table(op); host
 * operands keep the reference's own MPIR_Op_<op> loop, which beats an offload
 * below ~1 MiB (bench.py host_path.crossover).  Never initialises a GPU. */
int msx_operands_on_device(const void* in, const void* inout);
/* op_errno of the calling thread (Mpi.CallState->op_errno,
 * include/MpiCallState.h:13) and its reset (reduce.cpp:97, 3794) */
int msx_op_errno(void);
void msx_op_errno_reset(void);

/* inout[i] = inout[i] (op) in[i], i in [0,count); device pointers,
 * stream-ordered (returns after the launch, not after completion). */
int msx_reduce_local_dev(const void* in, void* inout, int64_t count,
                         MPI_Datatype datatype, MPI_Op op, void* stream);

/* Many small combines in as few launches as possible.  in, inout and counts
 * are HOST arrays of nseg entries; segment i is
 *   inout[i][k] = inout[i][k] (op) in[i][k], k in [0, counts[i])
 * on device pointers, one datatype and one op for the whole call.  The call is
 * stream-ordered on `stream` and returns after the enqueue; the three arrays
 * are read during the call only (the descriptors travel in the kernel
 * arguments), so the caller may overwrite them as soon as it returns.
 * The value: once the stream has drained, segment i holds exactly the bytes
 * msx_reduce_local_dev(in[i], inout[i], counts[i], datatype, op, stream) would
 * have produced, and no other byte of device memory is written.  Segments are
 * unordered among themselves and must be independent: `in` ranges may overlap
 * each other (one `in` may feed many segments), an `inout` range may meet no
 * other range of the call.
 * Builtin ops over every legal (op, predefined datatype) pair, MSX_FLOAT16 /
 * MSX_BFLOAT16 included; MSX_SUM_WIDE is MPI_SUM's combine.  User ops, host or
 * device, are MPI_ERR_OP.
 * Checks, all on the host before any GPU is touched, the first failure
 * deciding the class, nothing enqueued on a failure:
 *   1. nseg == 0: success;
 *   2. nseg < 0 or a null in / inout / counts array: MPI_ERR_ARG;
 *   3. an invalid op handle, an illegal (op, datatype) pair or a user op:
 *      MPI_ERR_OP;
 *   4. any counts[i] < 0: MPI_ERR_COUNT;
 *   5. a null in[i] or inout[i] with counts[i] > 0: MPI_ERR_BUFFER (segments
 *      with counts[i] == 0 are skipped, their pointers never looked at);
 *   6. in[i] == inout[i], or the byte range of inout[i] meeting its own in[i]
 *      range or any in[j] / inout[j] range, j != i: MPI_ERR_BUFFER, and
 *      msx_last_error() names both segments;
 *   7. no GPU: MPI_ERR_OTHER.
 * Segments below 16 MiB per operand whose operands share one offset from
 * 16-byte alignment are fused, up to *width per launch; operands at different
 * offsets are fused (element by element) below 64 KiB per operand; every other
 * segment is launched on its own, exactly as msx_reduce_local_dev launches it.
 *
 * msx_reduce_local_batch_plan runs checks 1 - 6 and reports what the call
 * would do, without ever initialising a GPU (a pure function of its
 * arguments; the addresses are never dereferenced): *width the most segments
 * one fused launch carries, *launches the kernel launches in all, *batched the
 * segments in fused launches, *single the segments launched on their own.
 * Empty segments count in neither.  A null output pointer is MPI_ERR_ARG. */
int msx_reduce_local_batch_dev(const void* const* in, void* const* inout, const int64_t* counts,
                               int nseg, MPI_Datatype datatype, MPI_Op op, void* stream);
int msx_reduce_local_batch_plan(const void* const* in, void* const* inout, const int64_t* counts,
                                int nseg, MPI_Datatype datatype, MPI_Op op,
                                int* width, int* launches, int* batched, int* single);

/* Device-resident user-defined reduction ops.
 *
 * A device user function: inout[i] = in[i] (op) inout[i] for i in [0,count),
 * MPI's operand order (`in` is the left operand), done by ENQUEUEING work on
 * `stream` (a hipStream_t).  in/inout are device-accessible.  For a derived
 * datatype they are the typed base addresses of `count` instances, as an
 * MPI_User_function gets them.  The function must not synchronise the stream
 * or the device and must not call MPI.  It may run on a library thread (the
 * engine worker, for non-blocking calls).  Returns MPI_SUCCESS or an MPI
 * error class, which fails the calling MPI call with that class.
 * include/msx_device_op.h is a kernel kit for writing one.
 *
 * msx_op_create_device returns a user-op handle (MPI_Op_commutative and
 * MPI_Op_free apply) that MPI_Reduce_local, msx_reduce_local_dev, MPI_Reduce,
 * MPI_Allreduce, MPI_Reduce_scatter[_block], MPI_Scan, MPI_Exscan and their
 * non-blocking forms accept; host buffers are staged to the GPU around the
 * calls.  Each collective evaluates the order of the host user-op path.
 * One-sided calls and intercommunicator reductions return MPI_ERR_OP; without
 * a GPU every use fails with MPI_ERR_OTHER and the function is never called. */
typedef int (MSX_Device_function)(const void* in, void* inout, int64_t count,
                                  MPI_Datatype datatype, void* stream, void* state);
int msx_op_create_device(MSX_Device_function* fn, int commute, void* state, MPI_Op* op);
/* 1 device op, 0 any other valid op, -1 invalid */
int msx_op_is_device(MPI_Op op);

/* The fused tree form of a device user op: ONE call evaluates the whole
 * reduction tree of a collective instead of p - 1 calls of the pairwise
 * function, so each contribution is read once and the result written once.
 *
 * A device tree function enqueues one evaluation on `stream` under the rules
 * of MSX_Device_function (no synchronisation, no MPI calls, possibly on a
 * library thread).  The slot layout is msx_reduce_tree_spec_dev's: P leaves (a
 * power of two <= 16) in 2P slots, leaf k in srcs[2k] and, when bit k of
 * pairmask is set, its fold pair in srcs[2k+1]; leaves >= nleaves are absent
 * (nleaves == 0: all present); with chain != 0, P sources (2..16) in srcs[0..P),
 * pairmask == 0 and nleaves == 0.  srcs is a HOST array of device pointers
 * (typed bases for a derived datatype); slots of absent leaves and of unpaired
 * leaves are not to be read.  Sources are not written; `out` is one of the
 * sources or disjoint from all of them.
 *
 * The value is defined by the pairwise function g(in, inout) = fn's result:
 *   in_left == 0  leaf k = g(in = s[2k+1], inout = s[2k]) when paired, else
 *                 s[2k]; a node = g(in = right, inout = left); a node whose
 *                 right subtree is absent passes its left value up; a chain is
 *                 v = s[0], then v = g(in = s[k], inout = v), k = 1..P-1.
 *   in_left == 1  every role swapped: a pair = g(in = s[2k], inout = s[2k+1]),
 *                 a node = g(in = left, inout = right), a chain step
 *                 v = g(in = v, inout = s[k]).
 * Returns MPI_SUCCESS (enqueued), MSX_TREE_DECLINED (nothing enqueued: the
 * library runs the pairwise evaluation for that call) or an MPI error class,
 * which fails the calling MPI call.
 *
 * msx_op_create_device_tree registers fn (required) with tree_fn (NULL: the op
 * is exactly msx_op_create_device's).  MPI_Allreduce, MPI_Reduce and
 * MPI_Reduce_scatter[_block] and their non-blocking forms call tree_fn once
 * per evaluating rank when the shape fits 16 leaves (p <= 31 for the fold
 * trees, p <= 16 for binomial trees and chains); MPI_Scan / MPI_Exscan,
 * MPI_Reduce_local and larger shapes call fn as before.
 * include/msx_device_op.h: msx_kit::tree and MSX_DEVICE_OP_TREE write one. */
#define MSX_TREE_DECLINED (-1)
typedef int (MSX_Device_tree_function)(const void* const* srcs, int P, unsigned pairmask, int nleaves,
                                       int chain, int in_left, void* out, int64_t count,
                                       MPI_Datatype datatype, void* stream, void* state);
int msx_op_create_device_tree(MSX_Device_function* fn, MSX_Device_tree_function* tree_fn,
                              int commute, void* state, MPI_Op* op);
/* 1 device op with a tree function, 0 any other valid op, -1 invalid */
int msx_op_has_device_tree(MPI_Op op);
/* The op's tree function on the caller's memory and stream (tests and probes);
 * never the pairwise path.  Bad arguments are MPI_ERR_ARG before any GPU is
 * touched: null srcs or out, a tree P that is no power of two in 1..16, a
 * chain P outside 2..16, nleaves outside 0..P, pairmask bits at or above the
 * leaves present, a chain with a pairmask or nleaves, in_left not 0 or 1.  A
 * negative count is MPI_ERR_COUNT, an op without a tree function MPI_ERR_OP;
 * without a GPU MPI_ERR_OTHER and the function is never entered; count == 0
 * succeeds without a call; a decline is returned as MSX_TREE_DECLINED. */
int msx_reduce_tree_user_dev(const void* const* srcs, int P, unsigned pairmask, int nleaves, int chain,
                             int in_left, void* out, int64_t count, MPI_Datatype datatype, MPI_Op op,
                             void* stream);

/* packed[i*size + b] <- typed[i*extent + map(b)] for `count` instances of a
 * committed datatype (predefined or derived); typed is the buffer address the
 * type map is relative to.  Device pointers, stream-ordered. */
int msx_pack_dev(const void* typed, int64_t count, MPI_Datatype datatype, void* packed,
                 void* stream);
int msx_unpack_dev(const void* packed, int64_t count, MPI_Datatype datatype, void* typed,
                   void* stream);

/* A combine between two datatype layouts: MPI_Accumulate's origin and target
 * triples on device pointers, with no window.  Stream-ordered on `stream`; the
 * call returns after the enqueue, allocates nothing and never synchronises
 * (only the first GPU use of a type with an irregular type map uploads its run
 * table, once, as with msx_pack_dev).
 *
 * The value.  Let n be the number of basic elements of origin_count instances
 * of origin_type.  Element e of the origin is the e-th element of its type map
 * in type-map order, instances `extent` apart; the same holds for the target.
 * For e < n:
 *     target[e] = origin[e] (op) target[e]
 * the origin in the `in` role and the target in the `inout` role: the
 * reference's MPID_Uop_call(origin, target) of an accumulate (win.cpp:1435).
 * Equivalently, once the stream has drained the target holds the bytes of
 *     msx_pack_dev(origin), msx_pack_dev(target),
 *     msx_reduce_local_dev(in = packed origin, inout = the first n packed
 *     target elements), msx_unpack_dev
 * and no other byte of device memory is written.  MPI_REPLACE copies bytes
 * (the typed -> typed MPIR_Localcopy) and accepts any two committed types,
 * mixed structs included; MPI_NO_OP does nothing.  The origin may hold fewer
 * data bytes than the target (MPI's rule): the last target instance is then
 * partly covered.  The spans of the two operands may overlap (two columns of
 * one matrix); the result is defined when no target-mapped byte among the n
 * elements is an origin-mapped byte and the target map names no location
 * twice.
 *
 * Checks, all on the host before any GPU is touched, the first failure
 * deciding the class, nothing enqueued on a failure:
 *   1. either count negative: MPI_ERR_COUNT;
 *   2. an invalid or uncommitted datatype: MPI_ERR_TYPE;
 *   3. an invalid op handle, a user op (host or device) or MSX_SUM_WIDE:
 *      MPI_ERR_OP;
 *   4. more origin data bytes than target data bytes: MPI_ERR_TRUNCATE (data
 *      bytes beyond 2^62 on either side: MPI_ERR_COUNT);
 *   5. zero origin data bytes, or MPI_NO_OP: success, the pointers are never
 *      looked at;
 *   6. for any op except MPI_REPLACE the two types must share one basic
 *      element type: a type with none (a mixed struct, the pair types
 *      MPI_FLOAT_INT .. MPI_LONG_DOUBLE_INT) or two element types of different
 *      kinds: MPI_ERR_TYPE; an (op, element type) pair outside the op's table:
 *      MPI_ERR_OP; a type map that splits an element: MPI_ERR_TYPE;
 *   7. a null origin or target: MPI_ERR_BUFFER;
 *   8. no GPU: MPI_ERR_OTHER.
 *
 * msx_accumulate_plan runs checks 1 - 6 and reports what the call would do,
 * without ever initialising a GPU (a pure function of its arguments; the call
 * itself dispatches on the same plan).  *elements: n.  *granule: the bytes one
 * work item moves when both bases are 16-byte aligned: the element size for an
 * op, for MPI_REPLACE the largest power of two <= 16 dividing every run offset
 * and length, the size and the extent of both layouts (0 with *path 0).
 * *path:
 *   0  nothing to do;
 *   1  both sides contiguous: msx_reduce_local_dev's kernel (the engine's copy
 *      kernel for MPI_REPLACE) on the two pieces;
 *   2  the origin contiguous and covering whole target instances: the
 *      derived-target accumulate of the one-sided path (msx_unpack_dev's
 *      kernel for MPI_REPLACE);
 *   3  MPI_REPLACE into a contiguous target: msx_pack_dev's kernel;
 *   4  the two-layout kernel: one launch that maps element e on both sides.
 * A null output pointer is MPI_ERR_ARG. */
int msx_accumulate_dev(const void* origin, int64_t origin_count, MPI_Datatype origin_type,
                       void* target, int64_t target_count, MPI_Datatype target_type,
                       MPI_Op op, void* stream);
int msx_accumulate_plan(int64_t origin_count, MPI_Datatype origin_type,
                        int64_t target_count, MPI_Datatype target_type, MPI_Op op,
                        int64_t* elements, int* path, int* granule);

/* A 16-bit float origin accumulated into an fp32 target in one launch: the
 * accumulator stays in fp32 and each bf16 / fp16 contribution is added as it
 * comes, rounded once, later, or never.  The triples are MPI_Accumulate's and
 * the element order is msx_accumulate_dev's.  The origin's basic element type
 * is MSX_FLOAT16 or MSX_BFLOAT16, the target's a 4-byte float (MPI_FLOAT,
 * MPI_REAL, MPI_REAL4); each side may be predefined or any committed derived
 * type over its element type.  Stream-ordered on `stream`; the call returns
 * after the enqueue, allocates nothing and never synchronises (only the first
 * GPU use of a type with an irregular type map uploads its run table, once, as
 * with msx_pack_dev).
 *
 * The value.  Let n be the number of basic elements of the origin triple.  For
 * e < n:
 *     target[e] = F_op(target[e], W(origin[e]))
 * the target in the `inout` role.  F_op is the fp32 combine of
 * msx_reduce_local_dev on MPI_FLOAT (the reference's op.cpp with the x86 NaN
 * rule for MPI_SUM / MPI_PROD, `inout > in ? inout : in` for MPI_MAX / MPI_MIN).
 * Ops: MPI_SUM, MPI_PROD, MPI_MAX, MPI_MIN; MPI_REPLACE is target[e] =
 * W(origin[e]), a typed widening copy; MPI_NO_OP does nothing.  No other byte
 * of device memory is written.  The target may hold more elements than n: the
 * rest is untouched, and a last target instance may be partly covered.  The
 * spans may interleave; the call is defined when no target-mapped byte among
 * the n elements is an origin-mapped byte and the target map names no location
 * twice.
 *
 * W widens exactly.  As bit patterns, uint16 x to uint32:
 *   MSX_BFLOAT16: x << 16, for every x;
 *   MSX_FLOAT16: the exact value for every non-NaN x, subnormals included; for
 *     a NaN (exponent 31, mantissa m != 0) sign << 31 | 0x7F800000 | m << 13:
 *     the payload and the signalling state are kept, it is not quieted.
 * So W is injective and narrowing W(x) gives x back for every non-NaN x.  The
 * NaN choice shows only where W(origin) itself is stored (MPI_REPLACE, MPI_MAX
 * / MPI_MIN choosing `in`); MPI_SUM / MPI_PROD quiet whatever NaN they return.
 *
 * Checks, all on the host before any GPU is touched, the first failure
 * deciding the class, nothing enqueued on a failure:
 *   1. either count negative: MPI_ERR_COUNT;
 *   2. an invalid or uncommitted datatype: MPI_ERR_TYPE;
 *   3. an invalid op handle, a user op (host or device), MSX_SUM_WIDE, or any
 *      builtin op other than the six above: MPI_ERR_OP;
 *   4. two times the origin's data bytes exceeding the target's data bytes:
 *      MPI_ERR_TRUNCATE (data bytes beyond 2^62 on either side: MPI_ERR_COUNT);
 *   5. zero origin data bytes, or MPI_NO_OP: success, the pointers are never
 *      looked at;
 *   6. an origin whose basic element type is neither MSX_FLOAT16 nor
 *      MSX_BFLOAT16, a target whose is not a 4-byte float, a type with no
 *      single element type (a mixed struct, the pair types), a type map that
 *      splits an element: MPI_ERR_TYPE;
 *   7. a null origin or target: MPI_ERR_BUFFER;
 *   8. no GPU: MPI_ERR_OTHER.
 *
 * msx_accumulate_widen_plan runs checks 1 - 6 and reports what the call would
 * do, without ever initialising a GPU (a pure function of its arguments; the
 * call itself dispatches on the same plan).  *elements: n.  *path:
 *   0  nothing to do;
 *   1  both pieces contiguous: the streaming kernel;
 *   2  the two-layout kernel (a contiguous side is a layout of one run).
 * A null output pointer is MPI_ERR_ARG. */
int msx_accumulate_widen_dev(const void* origin, int64_t origin_count, MPI_Datatype origin_type,
                             void* target, int64_t target_count, MPI_Datatype target_type,
                             MPI_Op op, void* stream);
int msx_accumulate_widen_plan(int64_t origin_count, MPI_Datatype origin_type,
                              int64_t target_count, MPI_Datatype target_type, MPI_Op op,
                              int64_t* elements, int* path);

/* Many msx_accumulate_dev calls of one builtin op in as few launches as
 * possible: the six typed accumulates of a 3-D block's halo sum in one launch.
 * All six arrays are HOST arrays of nseg entries; segment i is the origin
 * triple (origin[i], origin_count[i], origin_type[i]) into the target triple
 * (target[i], target_count[i], target_type[i]) on device pointers.  The call
 * is stream-ordered on `stream` and returns after the enqueue; the arrays are
 * read during the call only (the descriptors travel in the kernel arguments),
 * so the caller may overwrite them as soon as it returns.  It allocates nothing
 * and never synchronises (only the first GPU use of a type with an irregular
 * type map uploads its run table, once, as with msx_pack_dev).
 * The value: once the stream has drained, segment i's target holds exactly the
 * bytes
 *     msx_accumulate_dev(origin[i], origin_count[i], origin_type[i], target[i],
 *                        target_count[i], target_type[i], op, stream)
 * would have produced, and no other byte of device memory is written.
 * Segments are unordered among themselves.  The call is defined when no
 * target-mapped byte among a segment's n elements is a target-mapped or
 * origin-mapped byte of another segment, and each segment alone meets
 * msx_accumulate_dev's own condition.  Origins may overlap each other freely,
 * and spans may interleave (six faces of one array have overlapping spans and
 * disjoint maps), so spans are not compared; only check 9 looks at addresses.
 * Every builtin op msx_accumulate_dev accepts, MPI_REPLACE and MPI_NO_OP
 * included; user ops, host or device, and MSX_SUM_WIDE are MPI_ERR_OP.  For any
 * op except MPI_REPLACE / MPI_NO_OP all non-empty segments share one basic
 * element kind (one (op, kind) kernel runs per launch).
 * Checks, all on the host before any GPU is touched, the first failure
 * deciding the class, nothing enqueued on a failure; msx_last_error() names the
 * segment index of every per-segment failure:
 *   1. nseg == 0: success;
 *   2. nseg < 0 or any of the six arrays null: MPI_ERR_ARG;
 *   3. any count negative: MPI_ERR_COUNT;
 *   4. any datatype invalid or uncommitted: MPI_ERR_TYPE;
 *   5. an invalid op handle, a user op or MSX_SUM_WIDE: MPI_ERR_OP;
 *   6. per segment in index order, msx_accumulate_dev's checks 4 - 6:
 *      truncation MPI_ERR_TRUNCATE (data bytes beyond 2^62: MPI_ERR_COUNT); a
 *      segment with zero origin data bytes is empty and skipped from here on,
 *      its pointers never looked at; under MPI_NO_OP the call now succeeds;
 *      otherwise the element-type rules with msx_accumulate_dev's classes;
 *   7. for an op other than MPI_REPLACE, two non-empty segments of different
 *      element kinds: MPI_ERR_TYPE, naming both segments;
 *   8. a null origin or target of a non-empty segment: MPI_ERR_BUFFER;
 *   9. two non-empty segments with the same target address and the same target
 *      datatype handle (they certainly collide): MPI_ERR_BUFFER, naming both;
 *  10. no GPU: MPI_ERR_OTHER.
 * With nseg == 1 this is msx_accumulate_dev's class for every failing
 * argument set.
 * A non-empty segment is fused when its origin data bytes are below
 * *fuse_below and the 32-bit address map can hold it (both types' data sizes
 * below 4 GiB per instance), whatever path msx_accumulate_plan names for it: a
 * contiguous side is a layout of one run.  Fused segments fill launches in
 * index order, *width at a time; every other segment is launched on its own
 * where it stands, exactly as msx_accumulate_dev launches it.
 *
 * msx_accumulate_batch_plan runs checks 1 - 7 and reports what the call would
 * do, without ever initialising a GPU (a pure function of its arguments; it
 * takes no addresses): *width the most segments one fused launch carries,
 * *fuse_below the data-byte limit below which a segment is fused, *batched the
 * segments in fused launches, *single the segments launched on their own,
 * *launches = ceil(*batched / *width) + *single.  Empty segments count in
 * neither.  A null output pointer is MPI_ERR_ARG.  The call itself dispatches
 * on the same plan. */
int msx_accumulate_batch_dev(const void* const* origin, const int64_t* origin_count, const MPI_Datatype* origin_type,
                             void* const* target, const int64_t* target_count, const MPI_Datatype* target_type,
                             int nseg, MPI_Op op, void* stream);
int msx_accumulate_batch_plan(const int64_t* origin_count, const MPI_Datatype* origin_type,
                              const int64_t* target_count, const MPI_Datatype* target_type,
                              int nseg, MPI_Op op,
                              int* width, int64_t* fuse_below, int* launches, int* batched, int* single);

/* The combine that also hands back the old value, in ONE launch:
 * MPI_Fetch_and_op's value on device pointers, with no window.  For i < count:
 *     fetched[i] = inout[i]              (the old bytes, copied whole, the
 *                                         padding of a pair struct included)
 *     inout[i]   = inout[i] (op) in[i]
 * Stream-ordered on `stream`; returns after the enqueue, allocates nothing and
 * never synchronises.  Once the stream has drained, inout holds exactly the
 * bytes msx_reduce_local_dev(in, inout, count, datatype, op, stream) would have
 * produced and fetched the bytes inout had before; no other byte of device
 * memory is written.  The call moves 4 N bytes where msx_copy_dev +
 * msx_reduce_local_dev move 5 N in two launches.
 * Ops: every (builtin op, predefined datatype) pair msx_reduce_local_dev
 * accepts, MSX_FLOAT16 / MSX_BFLOAT16 and the pair types under MPI_MAXLOC /
 * MPI_MINLOC included; MSX_SUM_WIDE is MPI_SUM's combine; MPI_REPLACE
 * (inout[i] = in[i]) and MPI_NO_OP (inout unchanged; `in` is never looked at
 * and may be NULL) on any predefined datatype with data bytes.  User ops, host
 * or device, are MPI_ERR_OP.
 * Checks, all on the host before any GPU is touched, the first failure
 * deciding the class, nothing enqueued on a failure:
 *   1. count == 0: success;
 *   2. an invalid op handle, a user op or an illegal (op, datatype) pair:
 *      MPI_ERR_OP;
 *   3. a negative count: MPI_ERR_COUNT;
 *   4. a null inout or fetched, or a null in unless the op is MPI_NO_OP:
 *      MPI_ERR_BUFFER;
 *   5. in == inout: MPI_ERR_BUFFER;
 *   6. the byte range of fetched meeting the range of inout or of in:
 *      MPI_ERR_BUFFER, and msx_last_error() names the two operands;
 *   7. no GPU: MPI_ERR_OTHER.
 * The 16-byte vector body runs when in, fetched and inout share one offset
 * from 16-byte alignment (with head and tail elements in the same launch);
 * any other placement runs the whole call element by element.  There is no
 * realigning form as msx_reduce_local_dev has for two operands. */
int msx_fetch_and_op_dev(const void* in, void* fetched, void* inout, int64_t count,
                         MPI_Datatype datatype, MPI_Op op, void* stream);

/* Fetch and combine between three datatype layouts: MPI_Get_accumulate's
 * origin, result and target triples on device pointers, with no window.
 * Stream-ordered on `stream`; returns after the enqueue, allocates nothing and
 * never synchronises (only the first GPU use of a type with an irregular type
 * map uploads its run table, once, as with msx_pack_dev).
 *
 * The value.  Element e of a triple is defined as in msx_accumulate_dev.  Let
 * n be the number of basic elements of the origin triple; under MPI_NO_OP, of
 * the RESULT triple, and the origin triple (pointer, count and datatype) is
 * ignored entirely.  For e < n:
 *     result[e] = target[e]                 (the old value)
 *     target[e] = origin[e] (op) target[e]
 * the origin in the `in` role.  MPI_REPLACE: target[e] = origin[e], bytes, any
 * committed types; MPI_NO_OP leaves the target unchanged (MPI_Get).  Once the
 * stream has drained the target holds the bytes of msx_accumulate_dev(origin,
 * target) and the result the bytes of msx_accumulate_dev(MPI_REPLACE, target ->
 * result) taken before it; no other byte of device memory is written.  The
 * result and the target may each hold more data than the n elements; the rest
 * is untouched.  The spans may interleave; the call is defined when no
 * result-mapped byte among the n elements is an origin- or target-mapped byte,
 * no target-mapped byte is an origin-mapped byte, and neither the result map
 * nor the target map names a location twice.
 *
 * Checks, all on the host before any GPU is touched, the first failure
 * deciding the class, nothing enqueued on a failure:
 *   1. any count negative: MPI_ERR_COUNT;
 *   2. an invalid or uncommitted datatype: MPI_ERR_TYPE (the origin's is not
 *      checked under MPI_NO_OP);
 *   3. an invalid op handle, a user op (host or device) or MSX_SUM_WIDE:
 *      MPI_ERR_OP;
 *   4. the n elements' data bytes exceeding the target's or the result's data
 *      bytes: MPI_ERR_TRUNCATE (data bytes beyond 2^62: MPI_ERR_COUNT);
 *   5. zero bytes to move: success, the pointers are never looked at;
 *   6. for any op except MPI_REPLACE / MPI_NO_OP the three types must share one
 *      basic element kind, legal for the op, and no type map may split an
 *      element; the classes are msx_accumulate_dev's (MPI_ERR_TYPE, or
 *      MPI_ERR_OP for an illegal (op, element type) pair);
 *   7. a null result or target, or a null origin unless MPI_NO_OP:
 *      MPI_ERR_BUFFER;
 *   8. no GPU: MPI_ERR_OTHER.
 *
 * msx_get_accumulate_plan runs checks 1 - 6 and reports what the call would
 * do, without ever initialising a GPU (a pure function of its arguments; the
 * call itself dispatches on the same plan).  *elements: n.  *granule: the
 * element size for an op; for MPI_REPLACE / MPI_NO_OP the largest power of two
 * <= 16 dividing every run offset and length, the size and the extent of the
 * layouts involved (0 with *path 0).  *path:
 *   0  nothing to do;
 *   1  all three pieces contiguous: msx_fetch_and_op_dev's kernel (the engine's
 *      copy kernel for MPI_NO_OP);
 *   2  MPI_NO_OP, not all contiguous: msx_accumulate_dev(MPI_REPLACE, target ->
 *      result), with whatever path that plan takes (its two-layout kernel when
 *      the n elements end inside a target instance);
 *   3  the three-layout kernel: one launch that maps element e on all sides.
 * A null output pointer is MPI_ERR_ARG. */
int msx_get_accumulate_dev(const void* origin, int64_t origin_count, MPI_Datatype origin_type,
                           void* result, int64_t result_count, MPI_Datatype result_type,
                           void* target, int64_t target_count, MPI_Datatype target_type,
                           MPI_Op op, void* stream);
int msx_get_accumulate_plan(int64_t origin_count, MPI_Datatype origin_type,
                            int64_t result_count, MPI_Datatype result_type,
                            int64_t target_count, MPI_Datatype target_type, MPI_Op op,
                            int64_t* elements, int* path, int* granule);

/* out[i] = tree(srcs[0][i], ..., srcs[p-1][i]) with the balanced binary tree
 * ((s0 op s1) op (s2 op s3)) op ((s4 op s5) op (s6 op s7)), the left operand
 * of each combine in the reference's `inout` role.  p in {1,2,4,8,16};
 * srcs is a HOST array of device pointers; out may alias srcs[0]. */
/* SURVEY 8(e), the local reduce strong-scaled: inout[i] = inout[i] (op) in[i]
 * over one vector split into contiguous 256-byte-aligned ranges, one per GPU
 * of the node (ngpus <= 0: every visible GPU).  Host operands are pinned once
 * and each GPU combines its range in place over its own PCIe link; device
 * operands (and vectors under 1 MiB) stay on one GPU.  Blocking; MPI error
 * classes returned.  MSX_REDUCE_LOCAL_GPUS=k routes MPI_Reduce_local here. */
int msx_reduce_local_multi(const void* in, void* inout, int64_t count, MPI_Datatype datatype, MPI_Op op,
                           int ngpus);
int msx_reduce_tree_dev(const void* const* srcs, int p, void* out, int64_t count,
                        MPI_Datatype datatype, MPI_Op op, void* stream);

/* Any reference-order tree the engine evaluates: P leaves (power of two <= 16)
 * over srcs[2k] and, when bit k of pairmask is set, its fold pair srcs[2k+1]
 * (leaf k = op(srcs[2k] as inout, srcs[2k+1] as in)); leaves >= nleaves absent
 * (0 = all); or with chain != 0 the left-deep chain over srcs[0..P-1].
 * Stream-ordered, device pointers (tests and probes of the tree kernels). */
int msx_reduce_tree_spec_dev(const void* const* srcs, int P, unsigned pairmask, int nleaves, int chain,
                             void* out, int64_t count, MPI_Datatype datatype, MPI_Op op, void* stream);
/* The engine's local copy kernel (the collectives' collect step): dst <- src,
 * `bytes` bytes of device memory, stream-ordered (tests of the copy kernels). */
int msx_copy_dev(void* dst, const void* src, int64_t bytes, void* stream);
/* Tests of the engine's kernels in the launch forms only a collective uses.
 * Every pointer is device memory of the caller; the library allocates and
 * frees nothing.  Bad arguments (null arrays, nextra outside 0..31, nflags
 * outside 0..64, done_launches < 1 with a counter, a negative size, nseg
 * outside 0..32 for the push) return MPI_ERR_ARG before any GPU is touched.
 *
 * msx_reduce_tree_done_dev: msx_reduce_tree_spec_dev whose result also goes to
 * extra[0..nextra) and, with done_counter (a zeroed block of 1024 unsigned
 * words, left zero), is stored write-through and announced: once the
 * workgroups of `done_launches` launches on the block (this one included,
 * stream-ordered) have stored, done_seq is stored to every done_flags[i].
 * count == 0 launches nothing and counts no launch.
 * msx_push_dev: the GPU-flag schedules' push: segment i (below 4 GiB) to
 * dst[i] with write-through stores, then `seq` to every flags[i]; nseg == 0
 * posts the flags alone.  `counter` as above.  The launch's waiting workgroup
 * waits for nothing; wait_flags and wait_err name one device word each.
 * msx_copy_segs_dev: the engine's multi-segment copy, any nseg >= 0. */
int msx_reduce_tree_done_dev(const void* const* srcs, int P, unsigned pairmask, int nleaves, int chain,
                             void* out, void* const* extra, int nextra, unsigned* done_counter,
                             int done_launches, unsigned long long* const* done_flags, int done_nflags,
                             unsigned long long done_seq, int64_t count, MPI_Datatype datatype, MPI_Op op,
                             void* stream);
int msx_push_dev(const void* const* src, void* const* dst, const int64_t* nbytes, int nseg,
                 unsigned long long* const* flags, int nflags, unsigned long long seq, unsigned* counter,
                 const unsigned long long* wait_flags, int* wait_err, void* stream);
int msx_copy_segs_dev(const void* const* src, void* const* dst, const int64_t* nbytes, int nseg,
                      void* stream);
/* Test hook: pack / unpack geometry.  0 = by size (default: the one-wave tile
 * form when typed span + packed bytes exceed 512 MiB), 1 = always the
 * grid-stride form, 2 = always the tile form.  (The derived-target accumulate
 * always runs its tile form.)  The measurement kernels (HBM
 * probes, combine variants) live in the bench-only libmsx_probe.so. */
int msx_tune_pack(int mode);

/* host staging chunk size (bytes) for MPI_Reduce_local on host buffers */
int msx_set_staging_chunk(int64_t bytes);
/* host operands of MPI_Reduce_local: 0 (default) = pinned host memory is
 * combined in place by the kernel over PCIe (zero-copy), pageable memory of
 * at least 1 MiB is pinned for the call and combined
 * the same way (staged through HBM if the driver refuses to pin it);
 * 1 = every host operand is staged through HBM; 2 = pinned memory in place,
 * pageable memory staged */
int msx_set_host_mode(int mode);

/* schedule introspection for host-side tests of the collective engine
 * (mpid/reduce.cpp:3884-4066, 917-1334 restated as expression trees):
 * which = 0 allreduce tree of newrank n, 1 reduce_scatter tree of newrank n,
 * 2 pairwise chain of real rank n, 3 MPI_Reduce Rabenseifner tree of newrank n,
 * 4 MPI_Reduce binomial tree for root n.  src32[i] = real rank in kernel slot
 * i (-1 = empty).  The kernels' 16 leaves admit p <= 31 for the fold trees
 * (which = 0, 1, 3) and p <= 16 for the chain and the binomial tree; a larger
 * p is MPI_ERR_ARG. */
int msx_schedule_tree(int which, int p, int n, int* src32, int* P, unsigned* pairmask,
                      int* chain);
/* the spec a device-op collective hands to the op's tree function (a pure
 * function): which = 0 MPI_Allreduce for real rank n, 1 MPI_Reduce for root n,
 * 2 MPI_Reduce_scatter for real rank n (commutative: the recursive-halving tree
 * or the pairwise chain by the gate on total_count * type_size; non-commutative:
 * the allreduce of the whole vector).  src32[i] = real rank in slot i (-1 =
 * empty).  MPI_ERR_ARG when the shape does not fit 16 leaves (the collective
 * then keeps the pairwise evaluation) or p < 2. */
int msx_schedule_devop_tree(int which, int p, int n, int commutative, int64_t total_count, int type_size,
                            int* src32, int* P, unsigned* pairmask, int* nleaves, int* chain, int* in_left);
/* the pairwise calls that compute one rank's value of a collective with a
 * user-defined op, host function or device op (a pure function, any p >= 1):
 * which as above, and 3 MPI_Scan (exclusive = 1: MPI_Exscan) for real rank n.
 * Block r is rank r's contribution; step k is block steps[2k + 1] =
 * steps[2k] (op) it, the first `in`, the second `inout`; every block is an
 * operand exactly once, so the steps run in place.  *result: the block that
 * holds the value, -1 for rank 0 of an exscan.  p - 1 steps, at most p - 1 for
 * a scan.  MPI_ERR_ARG, with *nsteps set, when the plan has more than cap
 * steps (steps holds 2 * cap ints). */
int msx_schedule_userop_plan(int which, int p, int n, int commutative, int exclusive, int64_t total_count,
                             int type_size, int* steps, int cap, int* nsteps, int* result);
/* which = 0 allreduce, 1 reduce_scatter, 2 reduce: 0 recursive doubling,
 * 1 Rabenseifner, 2 recursive halving, 3 pairwise, 4 binomial */
int msx_schedule_algo(int which, int p, int64_t count, int type_size);
/* the same with the gate size taken from `dt`: MPI_Type_size (blocking calls,
 * reduce_scatter) or the extent (nbc = 1: the NBC task lists of
 * MPI_Iallreduce / MPI_Ireduce, reduce.cpp:4717,4881,6701,6740) */
int msx_schedule_algo_dt(int which, int p, int64_t count, MPI_Datatype dt, int nbc);
/* MPI_Ireduce's Rabenseifner tree of newrank n over root-relative ranks
 * (IreduceBuildScatterGatherTaskList, reduce.cpp:6267-6670) */
int msx_schedule_ireduce_tree(int p, int n, int root, int* src32, int* P, unsigned* pairmask,
                              int* chain);
int msx_schedule_newrank(int rank, int p);
/* the pipelined two-step allreduce's chunk plan for `rank` (tests): *chunk_el
 * elements per chunk; out[3i], out[3i+1], out[3i+2] = first element, end
 * element and owner newrank of each range of the rank's pieces over all
 * chunks; returns the range count, -1 if cap triples do not suffice */
int64_t msx_schedule_two_step(int p, int64_t count, int esz, int rank, int64_t* chunk_el, int64_t* out,
                              int64_t cap);
/* the same plan with chunks of chunk_el elements, the caller's choice (the
 * host-barrier Rabenseifner schedule cuts chunks of p sub-slots);
 * *chunk_el_out = chunk_el */
int64_t msx_schedule_pieces(int p, int64_t count, int64_t chunk_el, int rank, int64_t* chunk_el_out, int64_t* out,
                            int64_t cap);
int msx_schedule_block(int p, int64_t count, int n, int64_t* start, int64_t* len);

#ifdef __cplusplus
}
#endif
#endif
