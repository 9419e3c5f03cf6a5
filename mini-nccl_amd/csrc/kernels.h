// kernels.h -- host-side view of the HIP kernels in kernels.hip (launch wrappers only).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "p2p.h"

namespace mnccl {

// Element types the kernels are instantiated for (subset of ncclDataType_t values).
enum DType : int { kI32 = 2, kF16 = 6, kF32 = 7, kF64 = 8, kBF16 = 9,
                   // OCP fp8 (ncclFloat8e4m3 = e4m3fn, ncclFloat8e5m2): NCCL's and RCCL's values
                   kF8E4M3 = 10, kF8E5M2 = 11 };
enum RedOp : int { kSum = 0, kProd = 1, kMax = 2, kMin = 3,
                   // a handle of ncclRedOpCreatePreMulSum, resolved: the sum of inputs scaled by
                   // CollParams::scale where they enter a fold (kernels.hip Scale); the communicator
                   // calls only (launch_local_reduce refuses it)
                   kPreMulSum = 5 };

// Everything a ring / read kernel needs; passed by value as the kernel argument.
struct CollParams {
  const char* send;        // this rank's input (device)
  char* recv;              // this rank's output (device; may equal send)
  uint64_t chunk_bytes;    // (count / n) * elem_size
  uint64_t slice_bytes;    // payload bytes per channel message (<= slot_bytes)
  uint64_t slot_bytes;     // scratch slot stride (fixed per communicator: the configured slice)
  uint64_t nslices;        // ceil(chunk_bytes / slice_bytes)
  uint32_t iters;          // ceil(nslices / A): slices per pipeline of this call
  int32_t n, rank, nslots;
  char* scratch;           // this rank's scratch (regions per source rank)
  uint64_t* mbox;          // this rank's mailbox
  uint64_t* tx_seq;        // [peer][channel] messages sent so far (device, private)
  uint64_t* rx_seq;        // [peer][channel] messages received so far (device, private)
  char* peer_scratch[16];  // peers' scratch bases (IPC-mapped), indexed by rank
  uint64_t* peer_mbox[16]; // peers' mailboxes (IPC-mapped), indexed by rank
  uint32_t* status;        // host-mapped status word (kStatus* bits)
  const uint32_t* host_abort;  // host-mapped abort request
  uint32_t* started;       // host-mapped start word: the kernel writes call_seq when it begins
  uint32_t call_seq;       // this launch's sequence number (Comm::wait_for's deadline starts here)
  int32_t coll;            // schedule.h Coll (3 / 4: below): 0 all-reduce, 1 reduce-scatter (recv holds one chunk: the
                           // host passes recv - rank * chunk_bytes), 2 all-gather (send holds one
                           // chunk: the host passes send - rank * chunk_bytes), 5 all-to-all (a chunk is
                           // one block of the n in send and in recv), 7 gather (send shifted as
                           // the all-gather's), 8 scatter (recv shifted as the reduce-scatter's;
                           // a chunk is one block for both).  In what was padding:
                           // the struct's size and every other offset are the all-reduce's
  uint64_t timeout_ticks;  // s_memrealtime ticks (100 MHz)
  int32_t sys_fence;       // system-scope release fence before each ready flag
  int32_t pipes;           // the communicator's pipelines (mailbox / scratch / counter layout);
                           // a call's grid may run fewer (schedule.h call_pipelines)
  const char* peer_send[16];  // read schedule: every rank's send buffer, mapped here (own at [rank])
  const char* peer_recv[16];  // read schedule: every rank's recv buffer, mapped here
  uint64_t tail_bytes;        // bytes past n * chunk_bytes that the kernel copies send -> recv
                              // (the reference leaves them as its copy made them, api.cpp:173-175)
  uint32_t* claim;            // device word, 0 until the communicator's first give-up claims it:
                              // only that lane writes the status and its diagnostic
  uint32_t* go;               // device word: the read schedule's grid form -- call_seq once START
                              // is through (read_start_kernel), checked by the grid and DONE launches
  uint64_t sig;               // registered-window call (no host rendezvous): this call's signature,
                              // sent with START and compared with every peer's before any peer
                              // buffer is touched (0: a negotiated call, nothing to check)
  // the rooted collectives (coll 3 broadcast / 4 reduce): chunk_bytes is ceil(count / n) elements,
  // so the trailing chunks may be short or empty and every slice is clamped to the buffer's end
  // (schedule.h rooted_len); unused (0) by the other collectives
  uint64_t total_bytes;       // count * element size
  int32_t root;
  // kPreMulSum: the scalar's bits, one value of the call's datatype in the low bytes -- by value, so
  // the op may be destroyed once the call is issued (captured into a graph too); 0 and unread for
  // every other op.  After everything else: every other offset is what it was
  uint64_t scale;
};

constexpr int kMaxRanks = 16;
// The persistent collective kernels are built for at least this many resident waves per SIMD
// (__launch_bounds__: <= 256 registers per wave): a GPU keeps CUs x 4 SIMDs x this many of their
// waves resident at once, and every rank's pipeline w waits for its peers' pipeline w.
constexpr int kMinWavesPerSimd = 2;

// The persistent kernels: one launch per call, `channels` workgroups of `threads`.
enum PersistentKernel : int {
  kKernelRing,     // the ring schedule, every collective (p.coll picks the op table)
  kKernelRead,     // the read schedule's all-reduce
  kKernelOneshot,  // the one-shot all-reduce
  // the read schedule's two halves as collectives of their own (p.coll 1 / 2, the persistent form
  // and protocol of kKernelRead): scatter_fold folds chunk `rank` of every peer's send into recv;
  // gather_push stores send into chunk `rank` of every rank's recv (by element size: no arithmetic)
  kKernelScatterFold,
  kKernelGatherPush,
  // the read schedule's rooted collectives (p.coll 4 / 3; the same persistent form and protocol):
  // root_fold folds chunk `rank` of every rank's send into the ROOT's recv at the same offset (p.recv
  // is that buffer: the host passes its mapping of the root's recv on the other ranks); root_relay
  // copies chunk `rank` of the root's send into every rank's recv (by element size: no arithmetic)
  kKernelRootFold,
  kKernelRootRelay,
  // the read schedule's all-to-all (p.coll 5; the same persistent form and protocol; a chunk is one
  // block of the n in send and in recv): exchange_push stores block q of send into block `rank` of
  // rank q's recv, for every q (by element size: no arithmetic)
  kKernelExchangePush,
  // the read schedule's gather and scatter (p.coll 7 / 8; the same persistent form and protocol; a
  // chunk is one block): collect_push stores send into block `rank` of the ROOT's recv; deal_push,
  // on the root, stores block q of send into rank q's recv, for every q (by element size)
  kKernelCollectPush,
  kKernelDealPush,
};

// Launchers return hipSuccess or the launch error; dtype/op must be supported
// (checked by the caller).  vec = 16-byte path (all offsets 16-byte aligned).
// op: one of the four built-ins, or kPreMulSum for the kernels that fold (p.scale the scalar).
// launch_persistent refuses a p.coll that is not the kernel's, a root outside [0, n) for the
// rooted kernels (gather and scatter among them) and n < 2 for the all-to-all, the gather and the
// scatter; the kernels that only copy ignore op.
hipError_t launch_persistent(int kernel, int dtype, int op, bool vec, int channels, int threads,
                             const CollParams& p, hipStream_t stream);
// ncclAllToAllv on the read schedule (kernels.hip varblock_push): the per-destination blocks of this
// rank, a second by-value kernel argument (CollParams stays byte for byte what it was).  Indexed by
// destination rank q; this rank's own block at [rank].
struct VarBlockArgs {
  uint64_t src_off[16];  // byte offset of the block for q in this rank's send (sdispls[q] * element size)
  uint64_t dst_off[16];  // byte offset of that block in rank q's recv (rank q's rdispls[rank] * element size)
  uint64_t bytes[16];    // the block's length in bytes (0: nothing goes to q)
  uint32_t vec_mask;     // bit q: source and destination address are both dword-aligned (16-byte path)
  uint32_t pad;
};
// p: the all-to-all's geometry for chunk_bytes = the largest block of the whole matrix (the same on
// every rank), p.peer_recv every rank's recv.  By element size (1 / 2 / 4 / 8 from dtype): no arithmetic.
hipError_t launch_varblock(int dtype, int channels, int threads, const CollParams& p, const VarBlockArgs& v,
                           hipStream_t stream);
// mncclReduceScatterv / mncclAllGatherv on the read schedule (kernels.hip vhalf_fold / vhalf_push):
// this rank's block of the array-side buffers, a second by-value kernel argument (CollParams stays
// byte for byte what it was).  The arrays are the same on every rank, so `base` is the block's byte
// offset in EVERY rank's array-side buffer.
struct VHalfArgs {
  uint64_t base;   // displs[rank] * element size
  uint64_t bytes;  // counts[rank] * element size (0: this rank only takes part in the protocol)
};
// p: p.coll kCollReduceScatterV or kCollAllGatherV; the geometry for chunk_bytes = the call's largest
// block (the same on every rank); the one-block buffer's pointer shifted by -v.base (the fold's p.recv,
// the push's p.send), p.peer_send / p.peer_recv every rank's array-side buffer.  vec: this rank's
// alone (vhalves.h vhalf_vec).  The fold takes scatter_fold's datatypes and ops (p.scale the scalar of
// kPreMulSum); the push goes by element size (1 / 2 / 4 / 8 from dtype) and ignores op.
hipError_t launch_vhalf(int dtype, int op, bool vec, int channels, int threads, const CollParams& p, const VHalfArgs& v,
                        hipStream_t stream);
// ncclSend / ncclRecv (kernels.hip p2p_kernel): one launch for a whole group.  p: the communicator's
// mailbox, scratch, counters, control words and timeout as every kernel gets them (send / recv and
// the call geometry unused); a (p2p.h P2pArgs, a second by-value argument): per directed pair the
// operations in order, plus the self copies.  One 64-thread workgroup per wave: p2p_launch_waves(a)
// of them, wave b serving pair b / a.pipes on pipeline b % a.pipes.  Refuses an empty launch, more
// pairs or pipelines than the layout holds, and pairs on a communicator of one rank.
hipError_t launch_p2p(const CollParams& p, const P2pArgs& a, hipStream_t stream);
// The same group on a communicator with registered windows (kernels.hip p2p_window_group): every
// receiver posts a DEST record per message from the device, and the sender pushes straight into the
// recv buffer when that lies in a window, else through the scratch as above.  wa (p2p.h P2pWinArgs):
// the argument above plus, per recv entry, the window slot and offset it posts, the communicator's
// window table and the host-mapped mirror of its direct-send counters.  Refuses what launch_p2p
// refuses, a missing table and a slot outside it.
hipError_t launch_p2p_window(const CollParams& p, const P2pWinArgs& wa, hipStream_t stream);
// the read schedule's push form for large calls as three launches (start, grid fold, done):
// schedule.h read_grid_fits(p.chunk_bytes, p.n, kReadGridFloor) (2 <= n <= 8, whole 16-byte vectors), p.go set
// vectors: 0 = schedule.h read_grid_vectors; 1 / 2 / 4 (MINI_NCCL_GRID_VECTORS) for fp32 Sum only
hipError_t launch_read_grid(int dtype, int op, const CollParams& p, hipStream_t stream, int vectors = 0);
// out[i] = round(scale * in[i]) for i < count, one rounding in the datatype's arithmetic (a
// kPreMulSum call on a communicator of one rank); out may be in
hipError_t launch_scale(int dtype, void* out, const void* in, uint64_t count, uint64_t scale, hipStream_t stream);
// out[i] = op(local[i], incoming[i]) for i < count (the four built-in ops)
hipError_t launch_local_reduce(int dtype, int op, void* out, const void* local,
                               const void* incoming, uint64_t count, hipStream_t stream);

// Link probe: blocks spread over the `nremote` peers move `bytes` between `local` and each
// remote[d]: pushes (pull = false, the schedules' direction) or loads over the link (pull =
// true), with the remote side's cache policy `form`: kProbeSys = the hot path's 16-byte
// sc0 sc1 accesses, kProbeNt = non-temporal, kProbePlain = default policy.  Used to measure
// the xGMI bandwidth the schedules are bound by, and what other access forms would get.
enum : int { kProbeSys = 0, kProbeNt = 1, kProbePlain = 2 };
hipError_t launch_link_probe(char* local, char* const* remote, int nremote, uint64_t bytes, int form, bool pull,
                             hipStream_t stream);

// Loads the library's gfx950 code object onto the current device now (the runtime otherwise does it
// inside the process's first kernel launch, i.e. inside its first collective call: milliseconds of
// host time that grow with every kernel the library ships).  Best effort: an error is returned, not
// thrown, and the first launch then loads it as before.
hipError_t preload_kernels();

bool dtype_supported(int dtype);
int dtype_size(int dtype);

}  // namespace mnccl
