// msx_kernels.h — host-side launch interface of the gfx950 combine kernels.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "msx_types.h"

namespace msx {

// Completion counters of the engine's flag-posting kernels: a transport owns
// kCountBlocks blocks of kCountWords zeroed words (push_counter()): block 1 is
// k_push_wait's push, block 2 the two-step tree's result count (block 0 is
// unused).  Inside a block, word 0 is
// the top level, word 1 a launch count, and kCountSubs sub-counters sit 16
// words (64 B) apart from kCountSubBase (see count_done).
constexpr unsigned kCountSubs = 32;
constexpr unsigned kCountSubBase = 64;
constexpr unsigned kCountWords = 1024;
constexpr unsigned kCountBlocks = 4;

// Launch geometry of the streaming combine.
struct LaunchCfg {
    bool host = false;    // launched by the host-memory path of MPI_Reduce_local (zero-copy
                          // over PCIe, or a staged chunk): the k_combine_host symbol, so
                          // profiles keep the device-resident kernel's statistics apart
};

// inout[i] = op(inout[i], in[i]) for i in [0, count), stream-ordered on `s`.
// in / inout must be device-accessible from the current device.
// Returns hipSuccess, or hipErrorInvalidValue for a pair with no kernel.
hipError_t launch_combine(int opidx, Kind k, const void* in, void* inout, size_t count,
                          hipStream_t s, const LaunchCfg& cfg);

// Bytes per operand above which launch_combine (and launch_fetch_combine) take
// their DRAM-regime kernels (msx_kernels.hip; MSX_TEST_COMBINE_DRAM_MIN).
size_t combine_dram_min();

// The fetch form of the combine in ONE launch (msx_fetch.hip; msx.h,
// msx_fetch_and_op_dev): fetched[i] = inout[i], inout[i] = op(inout[i], in[i])
// for i in [0, count), launch_combine's geometry by size.  opidx may also be
// O_REPLACE (inout[i] = in[i]; k names the element size only).  `fetched`
// meets neither other operand.
hipError_t launch_fetch_combine(int opidx, Kind k, const void* in, void* fetched, void* inout, size_t count,
                                hipStream_t s);

// Many independent combines of one (op, kind) in ONE launch (k_combine_segs,
// msx_combine_segs.hip): segment i is inout[i] = op(inout[i], in[i]) over
// `count` elements, the bytes launch_combine gives.  At most
// kCombineSegsWidth segments, each below kCombineSegsMaxBytes per operand
// (larger ones keep launch_combine's own kernels); empty segments are skipped.
constexpr int kCombineSegsWidth = 128;
constexpr size_t kCombineSegsMaxBytes = (size_t)16 << 20;
struct CombineSeg {
    const void* in;
    void* io;
    size_t count;
};
hipError_t launch_combine_segs(int opidx, Kind k, const CombineSeg* segs, int nseg, hipStream_t s);

struct DevLayout;   // msx_dtype.h
// msx_pack.hip: packed <-> typed over `count` instances of one layout, and the
// per-element combine of packed elements into the typed side
hipError_t launch_dt_copy(const DevLayout& L, int64_t count, void* typed, void* packed, bool unpack,
                          hipStream_t s);
hipError_t launch_dt_acc(int opidx, Kind k, const DevLayout& L, int64_t count, const void* packed,
                         void* typed, hipStream_t s);
// msx_acc2.hip: n elements (a copy: `bytes` in granules of G) between two layouts
hipError_t launch_dt_acc2(int opidx, Kind k, const DevLayout& Lo, const void* origin, const DevLayout& Lt,
                          void* target, int64_t n, int align, hipStream_t s);
hipError_t launch_dt_copy2(const DevLayout& Lo, const void* origin, const DevLayout& Lt, void* target,
                           int64_t bytes, int G, hipStream_t s);
// msx_acc3.hip: the fetch forms over three layouts
hipError_t launch_dt_gacc3(int opidx, Kind k, const DevLayout& Lo, const void* origin, const DevLayout& Lr,
                           void* result, const DevLayout& Lt, void* target, int64_t n, int align, hipStream_t s);
hipError_t launch_dt_xchg3(const DevLayout& Lo, const void* origin, const DevLayout& Lr, void* result,
                           const DevLayout& Lt, void* target, int64_t bytes, int G, hipStream_t s);

// The two- and three-layout datatype kernels (msx_acc2.hip, msx_acc2_segs.hip,
// msx_acc3.hip) divide in 32 bits while the call's granule count and every
// side's instance size, in granules, are below 2^32 (the magic divisions of
// msx_dtype_map.h).
constexpr bool dt_map_narrow(int64_t n, int64_t gsize_o, int64_t gsize_t, int64_t gsize_r = 0)
{
    return n < 0xffffffffll && gsize_o < 0xffffffffll && gsize_t < 0xffffffffll && gsize_r < 0xffffffffll;
}

// Many independent two-layout combines of one (op, kind) in ONE launch
// (k_dt_acc2_segs, msx_acc2_segs.hip; msx.h, msx_accumulate_batch_dev):
// segment i is target element e (op)= origin element e over the first `bytes`
// data bytes of its origin layout, the bytes launch_dt_acc2 gives.  A
// contiguous side is a regular layout of one run per instance.  At most
// kAcc2SegsWidth segments, each below kAcc2SegsFuseBelow data bytes and inside
// dt_map_narrow; empty segments are skipped.  align: the largest power of two
// dividing every element address of both sides of the segment (layouts and
// pointers); the launch runs its aligned form when every segment allows it.
// launch_dt_copy2_segs is MPI_REPLACE: bytes move in granules of the smallest
// `align` of the launch.
constexpr int kAcc2SegsWidth = 12;
constexpr int64_t kAcc2SegsFuseBelow = (int64_t)4 << 20;     // measured: DESIGN.md §3b
struct Acc2Seg {
    const DevLayout* lo;
    const void* origin;
    const DevLayout* lt;
    void* target;
    int64_t bytes;
    int align;
};
hipError_t launch_dt_acc2_segs(int opidx, Kind k, const Acc2Seg* segs, int nseg, hipStream_t s);
hipError_t launch_dt_copy2_segs(const Acc2Seg* segs, int nseg, hipStream_t s);

// The widening accumulate (msx_widen.hip; msx.h, msx_accumulate_widen_dev):
// inout[i] = F_op(inout[i], W(in[i])) for i in [0, count), `in` 16-bit floats
// of kind k (K_F16 / K_BF16), `inout` fp32, launch_combine's geometry by the
// target's size.  opidx: O_SUM, O_PROD, O_MAX, O_MIN or O_REPLACE (the
// widening copy).  Any byte alignment of either operand.
hipError_t launch_widen_combine(int opidx, Kind k, const void* in, void* inout, size_t count, hipStream_t s);
// The same between two layouts: target element e (op)= W(origin element e) for
// e < n in type-map order, 2-byte granules on the origin's map and 4-byte ones
// on the target's.  aligned: every origin element address is a multiple of 2
// and every target element address of 4 (layouts and pointers).
hipError_t launch_dt_accw2(int opidx, Kind k, const DevLayout& Lo, const void* origin, const DevLayout& Lt,
                           void* target, int64_t n, bool aligned, hipStream_t s);

// Reference-order tree combine over p inputs (p = 1..8):
//   out[i] = T(srcs[0][i], ..., srcs[p-1][i]) where T is the balanced binary
//   tree of the reference's recursive-halving/doubling schedules with the
//   left operand as `inout`:  ((s0 op s1) op (s2 op s3)) op ((s4 op s5) op ...)
// `srcs` is a device-visible array of p pointers (may be peer pointers).
// `out` may alias srcs[0].
hipError_t launch_tree(int opidx, Kind k, const void* const* srcs_dev, int p, void* out,
                       size_t count, hipStream_t s);

// General schedule-faithful combine (see k_tree in msx_kernels.hip):
//   chain == false: P (power of two <= 16) leaves; leaf i = src[2i] if bit i of
//     pairmask is clear, else src[2i] op src[2i+1] (the non-power-of-two fold);
//     then the balanced tree over the leaves, left operand = inout.
//   chain == true: ((src[0] op src[1]) op src[2]) ... op src[P-1], P <= 16.
struct TreeSpec {
    const void* src[32] = {};
    int P = 1;
    int nleaves = 0;        // 0 = P; else leaves [nleaves, P) are absent (binomial trees)
    unsigned pairmask = 0;
    bool chain = false;
    void* extra[31] = {};   // the result is also stored here (e.g. peers' windows)
    int nextra = 0;
    // Result-ready flags: when the tree workgroups of all `done_launches`
    // launches of one call (this one included; stream-ordered) have stored
    // their results, store done_seq to every done_flags[j] (system scope).
    // done_counter: a zeroed kCountWords block of the transport, left zero again.
    unsigned* done_counter = nullptr;
    unsigned done_launches = 1;
    int done_nflags = 0;
    unsigned long long* done_flags[64] = {};
    unsigned long long done_seq = 0;
};
hipError_t launch_tree_spec(int opidx, Kind k, const TreeSpec& t, void* out, size_t count,
                            hipStream_t s);

// Store `seq` to *dst[i] for i < n (system scope), in stream order after the
// launches before it (flags that announce no data of their own).
hipError_t launch_post_flags(unsigned long long* const* dst, int n, unsigned long long seq, hipStream_t s);

// The GPU-flag schedules' synchronisation point, one launch: copy nseg ranges
// (each below 4 GiB) into peer windows with write-through stores and, once
// every workgroup's stores completed, store `seq` to every flags[i] (nseg may
// be 0: the flags are then posted by the waiting workgroup itself); plus ONE
// workgroup that waits until wait_flags[r] >= seq for r < wait_n, r !=
// wait_skip (flag_wait_seconds() bound, then wait_tag * 65536 + 1 + r ->
// *wait_err).  Launches after it on `s` read what the flags announce.
// `counter`: a zeroed kCountWords block of the caller's transport (left zero
// again); launches sharing one counter must not overlap.
hipError_t launch_push_wait(const void* const* src, void* const* dst, const size_t* nbytes, int nseg,
                            unsigned long long* const* flags, int nflags, unsigned long long seq,
                            unsigned* counter, const unsigned long long* wait_flags, int wait_n, int wait_skip,
                            int* wait_err, hipStream_t s, int wait_tag = 1);
// Bound of every GPU flag wait: MSX_FLAG_TIMEOUT_MS (default 20000), in
// s_memrealtime ticks and in seconds.
unsigned long long flag_wait_ticks();
double flag_wait_seconds();

// Copy nseg independent byte ranges in one launch (one grid row per segment),
// used to pull allgather blocks from every peer concurrently.
hipError_t launch_copy_segs(const void* const* src, void* const* dst, const size_t* nbytes,
                            int nseg, hipStream_t s);

// pack/unpack geometry (test hook, msx_tune_pack): 0 by size, 1 grid-stride
// form, 2 tile form (msx_pack.hip); the accumulate always runs its tile form
int pack_tune_set(int mode);

}  // namespace msx
