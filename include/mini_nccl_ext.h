/*
 * mini_nccl_ext.h -- MI355X-build extensions next to the drop-in ABI.
 *
 * Nothing here is needed to use the library as a drop-in for the reference; these
 * entry points expose the hot path's pieces for measurement and diagnostics:
 *
 *   mncclLocalReduce     the ★ scatter-reduce element-wise kernel on its own
 *                        (reference elementwise_reduce_kernel, mini_nccl.cu:43-47):
 *                        out[i] = op(local[i], incoming[i]); the 1-GPU "local reduce"
 *                        workload of BASELINE.md and bench.py at N = 1.
 *   mncclCommGetAsyncError  sticky error of a communicator (a timed-out or aborted
 *                        all-reduce leaves the ring state inconsistent; every later
 *                        call returns this error), like NCCL's ncclCommGetAsyncError.
 *   mncclCommGetInfo     resolved configuration of a communicator (mncclCommGetInfoV: the
 *                        caller states its struct's size, so an older caller is never
 *                        written past its end; mncclCommGetInfo writes the pre-300 prefix).
 *   mncclCommSetAlgo     choose the schedule for later calls (same association order).
 *   mncclCommLinkProbe   measure the xGMI write bandwidth the schedules are bound by.
 *
 * and the two halves of the all-reduce under NCCL's names and signatures, so that an NCCL / RCCL
 * caller that shards its state recompiles unchanged (the reference has neither: mini_nccl_api.h
 * stays its six entry points):
 *
 *   ncclReduceScatter    recv = chunk `rank` of what ncclAllReduce would produce over send's
 *                        nranks * recvcount elements, bit for bit.
 *   ncclAllGather        recv = every rank's send, rank q's at element q * sendcount.
 *
 * and NCCL's two rooted collectives:
 *
 *   ncclBroadcast        every rank's recv = the root's send.
 *   ncclReduce           the root's recv = the reduction of every rank's send (ncclAllReduce's bits
 *                        when count is a multiple of nranks); nobody else's recv is touched.
 *
 * and RCCL's dense exchange:
 *
 *   ncclAllToAll         block q of rank r's send becomes block r of rank q's recv, byte for byte.
 *   ncclAllToAllv        the same exchange with a count and a displacement per peer on both sides
 *                        (expert-parallel dispatch / combine: every rank sends every peer a different
 *                        number of tokens, possibly none).
 *
 * and the all-reduce's halves with per-rank counts, which neither NCCL nor RCCL has (callers there
 * compose them from broadcasts / reduces inside one group, which this library does not take), under
 * the library's prefix and in MPI's argument order (data-parallel attention in front of
 * expert-parallel MLPs, FSDP-style sharding of a dimension the rank count does not divide):
 *
 *   mncclAllGatherv      every rank's recv gets rank q's send at elements [rdispls[q], + recvcounts[q]).
 *   mncclReduceScatterv  rank r's recv = the reduction over all ranks of elements [sdispls[r],
 *                        + sendcounts[r]) of their send, in ncclReduceScatter's association.
 *
 * and RCCL's rooted data movers (torch.distributed.gather / scatter, metrics or KV blocks collected
 * on one rank, shards dealt out of one rank):
 *
 *   ncclGather           the root's recv = every rank's send, rank q's at element q * sendcount.
 *   ncclScatter          rank q's recv = block q of the root's send.
 *
 * and NCCL's point-to-point calls (pipeline parallelism, halo exchanges, batch_isend_irecv):
 *
 *   ncclSend / ncclRecv  `count` elements from one rank to another, byte for byte, with no host
 *                        rendezvous: two ranks exchange while the others do nothing.
 *   ncclGroupStart / ncclGroupEnd   several sends and recvs as one launch in which all progress
 *                        concurrently.
 *
 * and NCCL's user-created reduction op (gradient averaging, a loss scale folded into the reduction):
 *
 *   ncclRedOpCreatePreMulSum / ncclRedOpDestroy   a sum whose inputs are multiplied by one scalar on
 *                        their way into the fold, inside the reducing kernels.
 */
#ifndef MINI_NCCL_EXT_H_
#define MINI_NCCL_EXT_H_

#include "mini_nccl_api.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mncclVersion() of the library this header describes, 10000*major + 100*minor + patch:
   300 mncclCommInfo_t grew (mncclCommGetInfoV); 301 user buffers shared as dma-bufs,
   MINI_NCCL_TUNE removed; 400 the direct schedule and MINI_NCCL_PULL / DIRECT_OVERLAP /
   CALIBRATE / PIPE_DEPTH / MIN_SLICE / STAGE_HOST removed, MINI_NCCL_READ_PUSH added, the ring
   runs only the pipelines a call's slices need, mncclCommInfo_t grew again (same prefix);
   401 the one-shot schedule (mncclAlgoOneShot; auto's small calls that would run the ring);
   500 auto runs the read schedule only where every pair of GPUs is one xGMI hop apart (or
   shares a GPU), mncclCommInfo_t grew (same prefix: auto_read, peer_link / peer_hops,
   auto_reason, read_grid_calls, window_calls, windows, auto_grid), mncclAlgoReadGrid, registered windows
   (mncclCommRegister / mncclCommDeregister: read calls with no host rendezvous);
   501 imports of a same-GPU peer's memory are never unmapped while the process lives (the GPU
   driver's handle loss), mncclCommInfo_t grew (same prefix: retired_imports), auto's
   large read calls take the grid form wherever it fits (co-located ranks too);
   600 the read schedule's load form and MINI_NCCL_READ_PUSH removed (read_push is always 1), a
   byte budget on retired same-GPU imports (MINI_NCCL_RETIRED_MB; mncclCommInfo_t grew, same
   prefix: retired_bytes, retired_budget, budget_refusals, window_fast, run_pipelines), window calls carry the
   schedule choice in their signature and skip the host rendezvous only when no two ranks share a
   GPU (MINI_NCCL_WINDOW_RENDEZVOUS); still 600: ncclReduceScatter and ncclAllGather were added
   without a change to anything above -- a caller detects them by symbol; still 600: ncclBroadcast
   and ncclReduce were added the same way; still 600: ncclAllToAll was added the same way; still 600:
   ncclAllToAllv was added the same way (detected by symbol); still 600: ncclSend, ncclRecv,
   ncclGroupStart and ncclGroupEnd were added the same way; still 600: ncclRedOpCreatePreMulSum and
   ncclRedOpDestroy were added the same way; still 600: ncclGather and ncclScatter were added the
   same way (detected by symbol); still 600: ncclSend / ncclRecv push straight into a recvbuff that
   lies in a registered window (no new symbol; mncclCommInfo_t grew, same prefix: p2p_direct_recvs,
   p2p_direct_sends -- mncclCommGetInfoV writes them to a caller whose struct has room); still 600:
   mncclAllGatherv and mncclReduceScatterv were added the same way (detected by symbol;
   mncclCommInfo_t did not grow) */
#define MNCCL_VERSION 600

/* schedules; all produce bit-identical results (same fold order per element) */
typedef enum {
  mncclAlgoAuto = -1,  /* the library's default: read for device buffers every rank can share
                          when every pair of GPUs is one xGMI hop apart (or shares a GPU: see
                          mncclCommInfo_t.auto_read) -- its large calls in the grid form (since 501
                          wherever they fit it, co-located ranks too; 500: only when every rank had
                          a GPU of its own), the rest persistent; every other call one-shot when at
                          most 64 KiB, else the ring */
  mncclAlgoRing = 0,   /* the reference's ring: neighbour r -> r+1, 2(n-1) steps */
  mncclAlgoDirect = 1, /* removed in 400 (never faster than the ring); mncclCommSetAlgo and
                          MINI_NCCL_ALGO reject it */
  mncclAlgoRead = 2    /* no scratch: rank c loads the peers' slices of chunk c straight from
                          their send buffers (mapped per allocation, negotiated per call) and
                          folds them in the same order, then stores the result into its own
                          recv AND into every peer's recv -- the peers write chunk c of YOUR
                          recv during the call, and those writes are visible to your stream's
                          work after the call.  A call whose buffers some rank
                          cannot share (host memory, a full export table) runs the ring
                          instead, on every rank alike */,
  mncclAlgoOneShot = 3 /* since 401, small calls: every rank stores its whole input into every
                          peer's scratch in one message per pipeline and folds all n chunks
                          itself in the same order -- one hand-off instead of the ring's
                          2(n-1).  mncclAlgoAuto takes it for calls of at most 64 KiB that the
                          read schedule cannot take (host buffers, a full export table); forced,
                          every call whose pieces fit one round of the pipelines (the others run
                          as with mncclAlgoAuto) */,
  mncclAlgoReadGrid = 4 /* since 500: mncclAlgoRead with its large calls (chunks of >= 4 MiB, whole
                           16-byte vectors, up to 8 ranks, push form) launched as a one-wave START,
                           a grid of one-batch fold workgroups and a one-wave DONE instead of the
                           persistent kernel; the same bits.  A runtime form for the node to
                           measure beside the default (mncclCommInfo_t.read_grid_calls) */
} mncclAlgo_t;

typedef struct {
  int rank, nranks, device;
  size_t slice_bytes;     /* MINI_NCCL_SLICE_SIZE: bytes per channel message */
  int window;             /* MINI_NCCL_WINDOW_SIZE \ pipelines x slots <= WINDOW x SIGNAL_BATCH: the  */
  int signal_batch;       /* MINI_NCCL_SIGNAL_BATCH / reference's bound on messages in flight per link */
  int channels;           /* workgroups of the persistent kernel; each wave is one pipeline */
  int slots;              /* scratch slots per channel (2 = the reference's double buffer) */
  int threads;            /* threads per workgroup */
  int algo;               /* mncclAlgo_t used by ncclAllReduce */
  int blocking;           /* MINI_NCCL_BLOCKING */
  int sys_fence;          /* MINI_NCCL_SYS_FENCE: system-scope release fence before each flag */
  double timeout_s;       /* MINI_NCCL_TIMEOUT_MS / 1000 */
  size_t scratch_bytes;   /* device scratch owned by this rank */
  double tune_ms[2];      /* always 0 since 301 (MINI_NCCL_TUNE was removed); kept for the
                             layout */
  int pipelines;          /* channels x threads / 64 */
  int ranks_on_device;    /* ranks of this communicator on this rank's GPU (itself included) */
  size_t slot_bytes;      /* largest payload per message (MINI_NCCL_SLICE_SIZE unless the
                             scratch cap MINI_NCCL_SCRATCH_MB shrank it) */
  int last_algo;          /* schedule the last all-reduce ran (mncclAlgo_t; -1: no kernel
                             yet): mncclAlgoRead falls back to the scratch schedule for a
                             call some rank's buffers cannot take part in */
  size_t peer_mappings;   /* peers' user allocations mapped into this process for the read
                             schedule (dma-buf imports of every communicator; csrc/ipcreg.h) */
  int scratch_algo;       /* the read schedule's fallback for calls whose buffers cannot be
                             shared: always the ring (mncclAlgoRing) */
  int calib_choice;       /* -1 since 400 (MINI_NCCL_CALIBRATE was removed); kept for the layout */
  double calib_ms[2];     /* 0 since 400; kept for the layout */
  /* since 300 */
  unsigned long long ipc_open_failures;  /* user-buffer imports that failed in this process */
  unsigned long long read_map_failures;  /* read calls this rank could not map (call fell back) */
  unsigned long long read_rounds;        /* read calls that needed the mapping round */
  unsigned long long closed_freed;       /* imports closed because their owner freed them */
  size_t live_exports;                   /* this process's user allocations exported and alive */
  /* since 400 */
  unsigned long long cap_refusals;       /* exports / imports refused because this process holds
                                            512 exports / 1024 imports already: each such call
                                            ran the ring (warned once per process) */
  unsigned long long liveness_queries;   /* pointer queries this process made to find freed
                                            exports (per call: the call's own buffers + at most
                                            4 others) */
  int read_push;                         /* always 1 since 600 (the load form and MINI_NCCL_READ_PUSH
                                            were removed); kept for the layout */
  /* since 500 */
  int auto_read;                         /* 1: the topology lets auto run the read schedule (every pair
                                            of ranks shares a GPU or is one xGMI hop apart; the
                                            same on every rank); 0: auto runs the ring */
  int peer_link[16];                     /* how this rank's GPU reaches rank q's: -1 the same GPU,
                                            -2 unknown (not visible here), else the runtime's link
                                            type (hipExtGetLinkTypeAndHopCount: 2 PCIe, 4 xGMI) */
  int peer_hops[16];                     /* hop count of that link (0 for the same GPU) */
  char auto_reason[160];                 /* the rule's verdict in words (NUL-terminated) */
  unsigned long long read_grid_calls;    /* calls this communicator ran in the read schedule's grid
                                            form (mncclAlgoReadGrid) */
  unsigned long long window_calls;       /* calls launched on registered windows: no host rendezvous */
  int windows;                           /* windows registered on this communicator */
  int auto_grid;                         /* 1: auto launches large read calls in the grid form
                                            (mncclAlgoReadGrid's; since 501 whenever auto runs the
                                            read schedule in its push form) */
  /* since 501 */
  int retired_imports;                   /* process-wide: peers' freed allocations on this GPU still
                                            mapped here (same-GPU ranks only; held until the process
                                            exits -- DESIGN.md, Same-GPU handle loss) */
  /* since 600 */
  unsigned long long retired_bytes;      /* process-wide: bytes those retired imports keep mapped */
  unsigned long long retired_budget;     /* MINI_NCCL_RETIRED_MB in bytes (default: 1/8 of this GPU's
                                            memory / the ranks on it): once retired_bytes reaches it, a call that would
                                            map a new buffer of a same-GPU peer runs the ring instead
                                            (on every rank alike) */
  unsigned long long budget_refusals;    /* process-wide: same-GPU imports refused by that budget (each
                                            such call ran the ring; warned once per process) */
  int window_fast;                       /* 1: calls on registered windows launch with no host
                                            rendezvous (MINI_NCCL_WINDOW_RENDEZVOUS=0, or auto when
                                            no two ranks share a GPU); 0: they are negotiated like
                                            other calls (co-located ranks meet faster on the host) */
  int run_pipelines;                     /* the pipelines a call may launch: `pipelines`, capped so
                                            that the waves of every rank sharing a GPU stay resident
                                            together (CUs x 4 SIMDs x 2 waves / ranks on the most
                                            crowded GPU) */
  /* still 600: point to point on registered windows (ncclSend / ncclRecv, Transport) */
  unsigned long long p2p_direct_recvs;   /* ncclRecv operations this rank posted as direct (recvbuff in
                                            a registered window with a table slot): counted on the
                                            host when the launch is issued, so exact at once */
  unsigned long long p2p_direct_sends;   /* messages this rank's kernels pushed straight into a peer's
                                            recvbuff: counted on the device and mirrored into a
                                            host-mapped page by the kernel, so exact once every call
                                            issued so far has completed (after a blocking call
                                            returned, or the stream was synchronized) */
} mncclCommInfo_t;

/* The all-reduce's two halves, NCCL's signatures.  ncclReduceScatter: sendbuff holds nranks *
 * recvcount elements; rank r's recvbuff gets elements [r * recvcount, (r + 1) * recvcount) of what
 * ncclAllReduce would produce over them, bit for bit (the reference ring's association), so
 * ncclReduceScatter followed by ncclAllGather gives exactly ncclAllReduce's bits.  ncclAllGather:
 * recvbuff holds nranks * sendcount elements, rank q's sendbuff at [q * sendcount, (q + 1) *
 * sendcount), on every rank.  Datatypes and ops as ncclAllReduce (anything else: ncclInternalError);
 * argument checks, blocking mode, stream ordering, sticky errors and the watchdog as ncclAllReduce.
 * In place as NCCL defines it -- recvbuff == sendbuff + rank * recvcount elements, sendbuff ==
 * recvbuff + rank * sendcount elements; any other overlap of the two buffers is
 * ncclInvalidArgument (nothing is launched, the communicator stays usable).  Schedules: the read
 * schedule wherever ncclAllReduce's larger calls would run it (device buffers every rank can
 * share), else the ring's halves (the reduce-scatter with one extra hop, n instead of n - 1, to
 * land chunk r on rank r in the all-reduce's association); mncclCommInfo_t.last_algo reports
 * mncclAlgoRead or mncclAlgoRing.  No one-shot, grid or registered-window form: a call whose
 * buffers lie in windows is negotiated like any other.  Each GPU's memory moves n + 1 chunks per
 * call against the all-reduce's 2n. */
ncclResult_t ncclReduceScatter(const void* sendbuff, void* recvbuff, size_t recvcount, ncclDataType_t datatype,
                               ncclRedOp_t op, ncclComm_t comm, hipStream_t stream);
ncclResult_t ncclAllGather(const void* sendbuff, void* recvbuff, size_t sendcount, ncclDataType_t datatype,
                           ncclComm_t comm, hipStream_t stream);

/* The two rooted collectives, NCCL's signatures.
 * ncclBroadcast: every rank's recvbuff ends up holding the root's `count` elements of sendbuff.
 * sendbuff is read on the root only; elsewhere it is ignored and may be NULL.  In place on the root:
 * sendbuff == recvbuff.  Any datatype ncclAllGather takes (no arithmetic).
 * ncclReduce: the root's recvbuff ends up holding the reduction of every rank's `count` elements of
 * sendbuff.  recvbuff is written on the root only; elsewhere it is ignored, may be NULL and is never
 * touched.  In place on the root: recvbuff == sendbuff.  Datatypes and ops as ncclAllReduce.
 * Association: with q = ceil(count / nranks), chunk c is elements [c * q, min((c + 1) * q, count)) --
 * trailing chunks may be short or empty, and there is NO unreduced tail (ncclAllReduce's count %
 * nranks elements are the reference's quirk, not these calls') -- and every element of chunk c is
 * folded in ncclAllReduce's order for chunk c: acc = x_c, then acc = op(x_q, acc) for q = c + 1, ...,
 * c - 1 (mod nranks).  So when count % nranks == 0 the root's result is ncclAllReduce's, bit for bit,
 * and ncclReduce followed by ncclBroadcast from the same root gives it on every rank.  ncclBroadcast
 * moves its data by the same partition.
 * Argument checks, in this order: NULL comm: ncclInvalidArgument; count == 0: ncclSuccess (before the
 * datatype is looked at or the communicator read); an unsupported datatype / op: ncclInternalError;
 * then, with the communicator: root outside [0, nranks): ncclInvalidArgument; a NULL buffer this
 * rank's role needs (ncclBroadcast: recvbuff anywhere, sendbuff on the root; ncclReduce: sendbuff
 * anywhere, recvbuff on the root): ncclInvalidArgument; on the root, sendbuff and recvbuff overlapping
 * without being equal: ncclInvalidArgument.  In the last three nothing is launched or negotiated and
 * the communicator stays usable.  Ranks that disagree on the root or on the collective get
 * ncclInvalidUsage on every rank where the call is negotiated (the read schedule's rendezvous), the
 * communicator staying usable; no exception crosses the boundary.
 * Blocking mode, stream ordering, graph capture, sticky errors and the watchdog as ncclAllReduce;
 * nranks == 1 is a copy when the pointers differ.  Pinned host buffers go through their device
 * mapping, pageable ones through the stage (and cannot be captured).
 * Schedules: the read schedule where an all-reduce's larger calls would run it -- every rank folds
 * (ncclReduce), or copies out of the root's send (ncclBroadcast), chunk `rank` only and stores it
 * into the root's / every rank's recv, so the root's busiest link carries about 2 * bytes / nranks
 * where a root doing all the work would put all `bytes` on each of its links (a count derived from
 * the schedule: no run with ranks on distinct GPUs exists) -- otherwise the ring: a chain from the
 * root for ncclBroadcast, ncclAllReduce's ring with the other ranks' stores masked off for
 * ncclReduce.  mncclCommInfo_t.last_algo reports mncclAlgoRead or mncclAlgoRing.  No one-shot, grid
 * or registered-window form. */
ncclResult_t ncclBroadcast(const void* sendbuff, void* recvbuff, size_t count, ncclDataType_t datatype, int root,
                           ncclComm_t comm, hipStream_t stream);
ncclResult_t ncclReduce(const void* sendbuff, void* recvbuff, size_t count, ncclDataType_t datatype, ncclRedOp_t op,
                        int root, ncclComm_t comm, hipStream_t stream);

/* The all-to-all, RCCL's name and signature.  sendbuff and recvbuff each hold nranks * count
 * elements: block q of rank r's send, elements [q * count, (q + 1) * count), ends up as block r of
 * rank q's recv, byte for byte (no arithmetic: any datatype ncclAllGather takes; NaN payloads and
 * every other bit pattern survive); block `rank` of a rank's own send goes to block `rank` of its own
 * recv.  Checks, in this order: a NULL comm, sendbuff or recvbuff is ncclInvalidArgument; count == 0
 * is ncclSuccess; an unsupported datatype is ncclInternalError; any overlap of the two byte ranges
 * [buff, buff + nranks * count * size) -- sendbuff == recvbuff included: there is no in-place form,
 * as in RCCL, at any rank count -- is ncclInvalidArgument, with nothing launched or negotiated and
 * the communicator still usable.  Ranks that disagree on the collective, count or datatype get
 * ncclInvalidUsage wherever the call is negotiated, and the communicator stays usable.  Blocking
 * mode, stream ordering, graph capture, sticky errors, the watchdog and host buffers as for
 * ncclAllGather (two pageable buffers are staged side by side); nranks == 1 is one device copy.
 * Schedules: the read schedule where an all-reduce's larger calls would run it -- every rank pushes
 * block q of its send straight into rank q's recv, so every off-diagonal block crosses one link once
 * and all nranks - 1 links of a rank are busy for the whole call -- otherwise the ring, where the
 * block for the rank d places on travels d hops (nranks * (nranks - 1) / 2 messages per link and
 * iteration).  mncclCommInfo_t.last_algo reports mncclAlgoRead or mncclAlgoRing.  No one-shot, grid
 * or registered-window form. */
ncclResult_t ncclAllToAll(const void* sendbuff, void* recvbuff, size_t count, ncclDataType_t datatype, ncclComm_t comm,
                          hipStream_t stream);

/* Gather and scatter, RCCL's names and signatures.
 *
 * ncclGather: every rank's sendbuff holds sendcount elements; the root's recvbuff holds nranks *
 * sendcount, and rank q's block ends up at element q * sendcount of it, byte for byte.  recvbuff is
 * used on the root only: elsewhere it is ignored, may be NULL and is never touched.  In place on the
 * root: sendbuff == recvbuff + root * sendcount elements.
 * ncclScatter: the root's sendbuff holds nranks * recvcount elements and rank q's recvbuff gets block
 * q of it, byte for byte.  sendbuff is used on the root only: elsewhere it is ignored, may be NULL and
 * is never read.  In place on the root: recvbuff == sendbuff + root * recvcount elements.
 * No arithmetic: any datatype ncclAllGather takes, moved by element size; NaN payloads and every other
 * bit pattern survive.
 *
 * Checks, in this order (no exception crosses the boundary):
 *  1. a NULL comm: ncclInvalidArgument;
 *  2. a count of 0: ncclSuccess, before the datatype or the communicator is looked at;
 *  3. a group is open: ncclInvalidUsage, the group stays open and clean (no deferred collectives);
 *  4. an unsupported datatype: ncclInternalError, before the communicator is read;
 *  5. with the communicator, each ncclInvalidArgument with nothing launched or negotiated and the
 *     communicator still usable: root outside [0, nranks); a NULL buffer this rank's role needs
 *     (ncclGather: sendbuff everywhere and recvbuff on the root; ncclScatter: recvbuff everywhere and
 *     sendbuff on the root); on the root, byte ranges that overlap without being the in-place form.
 *     A non-root's unused buffer is not looked at at all;
 *  6. where the call is negotiated (the read schedule's rendezvous), ranks that disagree on the
 *     collective, count, datatype or root get ncclInvalidUsage on every rank and the communicator
 *     stays usable; on a forced ring these are the caller's to keep equal, as for ncclBroadcast.
 * nranks == 1 is one device copy when the pointers differ.  Blocking mode, stream ordering, graph
 * capture, sticky errors and the watchdog as for ncclBroadcast; pinned host buffers go through their
 * device mapping, pageable ones through the stage (in the in-place layout ncclAllGather uses) and
 * cannot be captured (ncclInvalidUsage).
 *
 * Schedules.  The read schedule where an all-reduce's larger calls would run it: column `root` and
 * row `root` of ncclAllToAll -- every rank pushes its one block straight into block `rank` of the
 * root's recvbuff (ncclGather), the root pushes block q of its sendbuff straight into rank q's
 * recvbuff (ncclScatter).  Each block crosses one link once, all nranks - 1 links of the root are
 * busy for the whole call, nranks blocks move through the root's HBM and no scratch is used (derived
 * from the schedule, not measured: no run with ranks on distinct GPUs exists).  Otherwise the ring:
 * a chain in ring direction that ends (ncclGather) or starts (ncclScatter) at the root, the link
 * behind the root carrying nothing.  mncclCommInfo_t.last_algo reports mncclAlgoRead or
 * mncclAlgoRing.  No one-shot, grid or registered-window form: a call whose buffers lie in windows is
 * negotiated like any other and window_calls does not move. */
ncclResult_t ncclGather(const void* sendbuff, void* recvbuff, size_t sendcount, ncclDataType_t datatype, int root,
                        ncclComm_t comm, hipStream_t stream);
ncclResult_t ncclScatter(const void* sendbuff, void* recvbuff, size_t recvcount, ncclDataType_t datatype, int root,
                         ncclComm_t comm, hipStream_t stream);

/* The variable all-to-all, RCCL's name and signature.  Counts and displacements are in elements; the
 * four arrays are host arrays of nranks entries, read before the call returns (a captured call bakes
 * them into the graph).  Elements [sdispls[q], sdispls[q] + sendcounts[q]) of rank r's send become
 * elements [rdispls[r], rdispls[r] + recvcounts[r]) of rank q's recv, byte for byte; a rank's own
 * block goes from its send to its recv; bytes of recv outside every block are never written.
 * Datatypes as ncclAllToAll (no arithmetic: by element size).
 *
 * Checks, in this order (no exception crosses the boundary):
 *  1. a NULL comm or a NULL array: ncclInvalidArgument;
 *  2. an unsupported datatype: ncclInternalError, before the communicator is read;
 *  3. with the communicator, each ncclInvalidArgument with nothing launched or negotiated and the
 *     communicator still usable: a NULL sendbuff unless every sendcount is 0, a NULL recvbuff unless
 *     every recvcount is 0 (an idle rank may pass the NULL data pointer of an empty tensor for both);
 *     a displ + count or a byte size that overflows size_t; two non-empty recv blocks that overlap;
 *     a non-empty recv block that overlaps a non-empty send block (there is no in-place form).  Send
 *     blocks may overlap each other: they are only read;
 *  4. after the per-call rendezvous -- every rank sees every rank's counts -- sendcounts_r[q] !=
 *     recvcounts_q[r] for any pair: ncclInvalidUsage on every rank alike, nothing launched, the
 *     communicator still usable; the same when the ranks disagree on the collective or the datatype;
 *  5. nranks == 1: one device copy of block 0 (a count mismatch is still ncclInvalidUsage);
 *  6. every count on every rank 0: ncclSuccess, nothing launched.
 * A rank takes part in the rendezvous and the protocol even when all its own counts are 0: its peers
 * still exchange among themselves.  Blocking mode, stream ordering, sticky errors and the watchdog
 * as ncclAllToAll.
 *
 * Schedules.  Where every rank's buffers are device memory the peers can map: the read schedule, a
 * persistent kernel in ncclAllToAll's protocol whose geometry follows the LARGEST block of the whole
 * matrix; every block crosses one link once and no padding moves; a destination whose addresses are
 * dword-aligned on both sides goes in 16-byte vectors, any other element by element
 * (mncclCommInfo_t.last_algo: mncclAlgoRead).  Otherwise -- a forced ring, a topology that refuses
 * read, host buffers (pinned or pageable) -- the ring's ncclAllToAll on blocks PADDED to the largest
 * one, M rounded up to 16 bytes: the blocks are packed into a device stage, exchanged and unpacked
 * (last_algo: mncclAlgoRing).  That fallback costs 2 * nranks * Mpad bytes of device memory per
 * communicator and sends the padding over the links: a skewed matrix pays for its largest block
 * nranks - 1 times per rank.  The stage may have to be allocated, so a call captured into a HIP graph
 * cannot take the fallback: if it would and any rank's stream is capturing, every rank returns
 * ncclInvalidUsage with nothing launched.  A captured call on the read schedule replays correctly.
 * No one-shot, grid or registered-window form. */
ncclResult_t ncclAllToAllv(const void* sendbuff, const size_t sendcounts[], const size_t sdispls[], void* recvbuff,
                           const size_t recvcounts[], const size_t rdispls[], ncclDataType_t datatype, ncclComm_t comm,
                           hipStream_t stream);

/* The all-reduce's halves with per-rank counts.  Neither NCCL nor RCCL has them, so they carry the
 * library's prefix and MPI's argument order (MPI_Allgatherv / MPI_Reduce_scatter with displacements).
 * Counts and displacements are in elements; the two arrays are host arrays of nranks entries, read
 * before the call returns (a captured call bakes them into the graph).  Each call has an ARRAY side
 * with nranks blocks (mncclAllGatherv's recv, mncclReduceScatterv's send), block q at elements
 * [displs[q], displs[q] + counts[q]), and a SCALAR side, this rank's one block.
 *
 * mncclAllGatherv.  Rank q's `sendcount` elements end up at elements [rdispls[q], rdispls[q] +
 * recvcounts[q]) of every rank's recvbuff, byte for byte.  No arithmetic: any datatype ncclAllGather
 * takes, the fp8 types included, moved by element size.  Bytes of recvbuff outside every block are
 * never written.  In place: sendbuff == recvbuff + rdispls[rank] elements.
 *
 * mncclReduceScatterv.  Every rank's sendbuff holds block q at [sdispls[q], sdispls[q] +
 * sendcounts[q]); rank r's recvbuff gets the reduction of block r over all ranks in the all-reduce's
 * association for chunk r: acc = x_r, then acc = op(x_q, acc) for q = r+1 .. r-1 (mod nranks).  With
 * equal counts and contiguous displacements the result is ncclReduceScatter's, bit for bit, on every
 * schedule.  Datatypes and ops as ncclReduceScatter: the four built-in ops and
 * ncclRedOpCreatePreMulSum handles; the fp8 types, re-encoded after every step; ncclAvg and the
 * integer types other than ncclInt32 are ncclInternalError.  In place: recvbuff == sendbuff +
 * sdispls[rank] elements.
 *
 * Both.  The arrays must be IDENTICAL on every rank, and the scalar count must equal the array's
 * entry for `rank`: one byte offset then serves every peer's buffer.
 *
 * Checks, in this order (no exception crosses the boundary):
 *  1. a NULL comm or a NULL array: ncclInvalidArgument;
 *  2. a group open on this thread: ncclInvalidUsage, the group stays open and clean;
 *  3. an unsupported datatype or op: ncclInternalError, before the communicator is read (a user-op
 *     handle is looked up in the communicator afterwards, as in ncclReduceScatter);
 *  4. with the communicator: the sticky error first; then, each ncclInvalidArgument with nothing
 *     launched or negotiated and the communicator still usable: the scalar count differs from the
 *     array's entry for `rank`; a NULL data buffer on a side that has a non-zero count (a rank whose
 *     block is empty may pass NULL for its scalar side; both may be NULL when every count is 0); a
 *     displ + count or a byte size that overflows size_t; two non-empty blocks of the array side that
 *     overlap -- on BOTH calls: an in-place mncclReduceScatterv writes block `rank` of a buffer the
 *     peers are reading other blocks of; the scalar-side buffer overlapping any non-empty block
 *     without being the in-place form;
 *  5. after the per-call rendezvous -- every rank sees every rank's arrays -- ranks whose arrays
 *     differ in any entry: ncclInvalidUsage on every rank alike, nothing launched, the communicator
 *     still usable; the same when the ranks differ in the collective, the datatype, the op, a
 *     pre-multiplied sum's scalar bits or the schedule choice (mncclCommSetAlgo);
 *  6. every count 0 on every rank: ncclSuccess, nothing launched.  A rank whose own count is 0 still
 *     takes part in the rendezvous and the protocol;
 *  7. nranks == 1: one device copy when the pointers differ; for a pre-multiplied sum the scale
 *     kernel, as ncclReduceScatter at one rank.
 * Blocking mode, stream ordering, sticky errors and the watchdog as ncclReduceScatter / ncclAllGather.
 *
 * Schedules.  Where ncclAllToAllv would run the read schedule -- device buffers every rank can map,
 * a topology that allows read -- two persistent kernels in ncclReduceScatter's / ncclAllGather's
 * protocol whose geometry follows the LARGEST block, M = max(counts) * element size: rank r's slices
 * start at byte displs[r] * element size of the array-side buffers and are clamped to its own block,
 * so a rank with a short or empty block moves only what it has; no padding crosses a link and
 * nothing is packed.  The gather loads each slice of sendbuff once and stores it into its own and
 * every peer's recvbuff.  A rank takes the 16-byte path when every rank's buffers are dword-aligned
 * and its own block's byte offset and byte length are multiples of 4, the element path otherwise;
 * ranks of one call may differ in that, the bits do not (mncclCommInfo_t.last_algo: mncclAlgoRead).
 * Otherwise -- a forced ring, a topology that refuses read, host buffers (pinned or pageable) -- the
 * ring's halves on blocks PADDED to Mpad, M rounded up to 16 bytes, through a device stage of
 * nranks * Mpad bytes per communicator: the gather packs its block, runs the ring all-gather and
 * unpacks nranks blocks; the reduce-scatter packs nranks blocks, runs the ring reduce-scatter and
 * copies its block out; the padding's results are discarded (last_algo: mncclAlgoRing).  The stage
 * may have to be allocated, so a call captured into a HIP graph cannot take the fallback: if it would
 * and any rank's stream is capturing, every rank returns ncclInvalidUsage with nothing launched.  A
 * captured call on the read schedule replays correctly.  No one-shot, grid or registered-window form
 * (mncclCommInfo_t.window_calls does not move). */
ncclResult_t mncclAllGatherv(const void* sendbuff, size_t sendcount, void* recvbuff, const size_t recvcounts[],
                             const size_t rdispls[], ncclDataType_t datatype, ncclComm_t comm, hipStream_t stream);
ncclResult_t mncclReduceScatterv(const void* sendbuff, const size_t sendcounts[], const size_t sdispls[], void* recvbuff,
                                 size_t recvcount, ncclDataType_t datatype, ncclRedOp_t op, ncclComm_t comm,
                                 hipStream_t stream);

/* Point to point, NCCL's names and signatures.
 *
 * Data.  The `count` elements of an ncclSend arrive, byte for byte, in the matching ncclRecv on `peer`
 * (no arithmetic: any datatype ncclAllGather takes, by element size).  The sends from rank a to rank b
 * match the recvs on b from a in call order.  Count and datatype must agree on both ends, as in NCCL;
 * a disagreement is the caller's error and ends at the watchdog like any other stuck call.
 *
 * Groups.  Group state is per thread and groups nest by a depth counter.  An ungrouped ncclSend /
 * ncclRecv is a group of one.  Inside a group a call only records its operation and returns
 * ncclSuccess or its argument error; the outermost ncclGroupEnd launches every recorded operation as
 * ONE kernel launch in which all of them progress concurrently -- every directed pair (the sends to
 * one peer, the recvs from one peer) on waves of its own -- and then behaves exactly as a collective
 * does: blocking mode, stream ordering after the communicator's previous call, sticky errors, the
 * watchdog.  ncclGroupEnd with no open group is ncclInvalidUsage.  Every operation of a group must
 * name the same communicator and the same stream; one that does not is ncclInvalidUsage at that call.
 * Any error inside a group poisons it: ncclGroupEnd returns the first error, launches nothing, and
 * leaves the communicator usable.  A group may hold several sends to one peer and several recvs from
 * one peer: they run in call order.  At most 64 operations fit in a group (kMaxGroupOps); one more is
 * ncclInvalidUsage.  DEFERRED COLLECTIVES ARE OUT OF SCOPE: ncclAllReduce, ncclReduceScatter,
 * ncclAllGather, ncclBroadcast, ncclReduce, ncclAllToAll, ncclAllToAllv, ncclGather, ncclScatter, mncclAllGatherv or
 * mncclReduceScatterv called while a group is open
 * return ncclInvalidUsage (after their NULL and count == 0 checks) with nothing launched, and the
 * group stays open and clean; with no group open they behave exactly as before.
 *
 * Self.  Inside a group, a send to the own rank pairs with a recv from the own rank, in order: one
 * device copy inside the same launch.  Unequal byte sizes, or a self send or recv left unpaired at
 * ncclGroupEnd, is ncclInvalidUsage.  Outside a group peer == rank is ncclInvalidUsage, because it
 * could never complete.  With nranks == 1 only the self pair exists.
 *
 * Checks, in this order (no exception crosses the boundary):
 *  1. a NULL comm, or a NULL buffer with count != 0: ncclInvalidArgument;
 *  2. count == 0: ncclSuccess, nothing recorded and nothing moves -- both ends skip it, so matching
 *     stays consistent;
 *  3. an unsupported datatype: ncclInternalError, before the communicator is read;
 *  4. with the communicator, peer outside [0, nranks): ncclInvalidArgument;
 *  5. a byte size that overflows size_t: ncclInvalidArgument;
 *  6. a recv range overlapping another recv range, or any send range, of the same group:
 *     ncclInvalidArgument;
 *  7. a buffer that is neither device memory of this rank's GPU nor pinned host memory:
 *     ncclInvalidArgument.  Pinned host memory is reached through its device mapping.  PAGEABLE HOST
 *     MEMORY IS NOT STAGED for these calls.
 *
 * The deadlock rule, as NCCL states it.  Two ranks that each send to the other and then receive,
 * ungrouped, deadlock: they must put the send and the recv into one group.  An ungrouped ncclSend
 * returns (blocking mode), or its kernel ends (stream-ordered mode), only once its last slice is in
 * the receiver's scratch, and a message larger than the pair's scratch slots (slots x slot_bytes x the
 * message's pipelines) waits for the matching ncclRecv to drain them.  A shorter send MAY complete
 * before its recv is called; nothing promises it.
 *
 * Capture.  There is no host rendezvous and the message counters live on the device, so a group
 * captured into a HIP graph replays correctly; count, pointers and peers are baked into the graph.
 *
 * Transport.  The transfer runs the ring's scratch protocol between the two ranks -- the sender
 * stores slices of at most slot_bytes into its region of the receiver's scratch and raises READY, the
 * receiver copies them out and returns a CREDIT -- so mncclCommInfo_t.last_algo reports mncclAlgoRing.
 * A message's slices and pipelines are a function of its byte count and the communicator's
 * rank-uniform configuration only.
 *
 * Zero copy into registered windows.  On a communicator with AT LEAST ONE registered window
 * (mncclCommRegister) when ncclGroupEnd -- or the ungrouped call -- is made, the whole group runs a
 * second kernel with one more hand-off per message, made from the device: the receiver posts where
 * the bytes go, and the sender pushes them there.  An ncclRecv whose recvbuff range lies inside a
 * registered window is posted "direct" -- window, byte offset, byte count -- and the sender, which
 * has every window mapped since the collective registration, stores the message straight into
 * recvbuff: one pass over the bytes, no scratch, no host rendezvous, so idle ranks stay idle,
 * nothing blocks on the host and a captured group replays.  Any other recv (outside every window,
 * pinned host memory, or a window beyond the table's capacity: the point-to-point table holds the
 * first 16 live windows, slots assigned lowest-free-first on every rank alike) is posted "scratch"
 * and moves exactly as described above.  sendbuff may be anywhere.  Direct and scratch messages and
 * collectives follow each other on one pair in any order; the pushed bytes are visible to the
 * receiver's stream work after its call, plain loads included, as the read schedule's pushes are.
 * last_algo still reports mncclAlgoRing; mncclCommInfo_t.p2p_direct_recvs / p2p_direct_sends count
 * the direct operations.
 *   The switch is rank-uniform because registration is collective and ordered.  THE CALLER'S
 * OBLIGATION: a send and its matching recv are issued under the same set of registered windows --
 * they do not straddle an mncclCommRegister / mncclCommDeregister (and a captured group is replayed
 * under the windows it was captured with).  A pair that straddles one ends at the watchdog.
 *   With windows, the sender checks the receiver's record before it stores anything: the posted byte
 * count must equal its own (on the scratch path too), the window must be live on the sender and the
 * range must lie inside it.  A count disagreement between a send and its recv therefore FAILS FAST
 * -- ncclInvalidUsage on both ranks, sticky, nothing written outside the protocol words, as for a
 * broken window promise of ncclAllReduce -- instead of ending at the watchdog.  With windows a send,
 * direct or not, starts only once its recv has been issued and has posted: the deadlock rule above
 * then holds at every size (no short send completes early).  A group replayed from a HIP graph
 * advances p2p_direct_sends per replay and p2p_direct_recvs not at all (it is counted when the
 * group is issued).  With no window registered nothing changes: the first kernel runs exactly as
 * before. */
ncclResult_t ncclSend(const void* sendbuff, size_t count, ncclDataType_t datatype, int peer, ncclComm_t comm,
                      hipStream_t stream);
ncclResult_t ncclRecv(void* recvbuff, size_t count, ncclDataType_t datatype, int peer, ncclComm_t comm,
                      hipStream_t stream);
ncclResult_t ncclGroupStart(void);
ncclResult_t ncclGroupEnd(void);

/* Pre-multiplied sums (NCCL's ncclRedOpCreatePreMulSum / ncclRedOpDestroy: names, argument order and
 * enum values are NCCL's; detected by symbol, MNCCL_VERSION stays 600).  ncclAvg itself is still
 * rejected with ncclInternalError; an op created with the scalar 1 / nranks is its replacement.
 *
 * ncclRedOpCreatePreMulSum creates a reduction op of `comm` that ncclAllReduce, ncclReduceScatter and
 * ncclReduce accept wherever they accept ncclSum.  *scalar is ONE value of `datatype`, read on the
 * host before the call returns (ncclScalarHostImmediate, the only residence supported:
 * ncclScalarDevice is ncclInvalidUsage).  The handle written to *op is a value >= MNCCL_FIRST_USER_OP
 * that belongs to this communicator; at most 16 are live per communicator, and a destroyed handle's
 * value may be handed out again.  The scalar travels to the kernels BY VALUE in the launch arguments:
 * the op may be destroyed as soon as the last call using it has been issued -- with
 * MINI_NCCL_BLOCKING=0 before the call has run, and for a call captured into a HIP graph before the
 * graph is replayed.  mncclLocalReduce has no communicator and accepts the four built-in ops only.
 *
 * Result, bit for bit.  With s the scalar, every rank's input element x first becomes
 * y = round(s * x), ONE correctly rounded multiplication in the datatype's arithmetic: the IEEE
 * product for ncclFloat and ncclDouble; for ncclFloat16 and ncclBfloat16 the product, which is exact
 * in float, rounded to nearest even into the type; two's-complement wrap for ncclInt32.  The y are
 * then reduced exactly as ncclSum reduces them -- for chunk c, acc = y_c, then acc = y_q + acc for
 * q = c+1 ... c-1 (mod nranks) -- so the call equals the ncclSum call on buffers scaled beforehand,
 * on every schedule; the product and the sum are two roundings, never a fused multiply-add.  Two
 * things follow from the definition: ncclAllReduce's unreduced tail (count % nranks elements) keeps
 * the rank's own input UNSCALED, as it is outside the reduction; and with nranks == 1 the call is no
 * plain copy: recv = round(s * send) over all `count` elements, in place or not.
 *
 * THE SCALAR MUST BE THE SAME ON EVERY RANK.  NCCL permits a scalar per rank; this library does not:
 * on the read schedule rank c multiplies its peers' inputs with its own copy of the scalar.  Ranks
 * are compared by the op's kind and the scalar's bits, never by the handle's value, so they may
 * create their ops in different orders.  Wherever a call is negotiated (the read schedule's
 * rendezvous, ncclReduce's included) a difference is ncclInvalidUsage on every rank with nothing
 * written and the communicator still usable; on registered windows launched without a rendezvous the
 * scalar is part of the signature the kernels compare, with the consequences documented at
 * mncclCommRegister (ncclInvalidUsage on every rank, the communicator no longer usable).  The forced
 * ring negotiates nothing and cannot see a difference.
 *
 * Schedules.  The ring, the persistent read kernels, the grid form and the registered-window launch
 * apply the scale inside their folds: no extra pass over the buffer.  The one-shot schedule has no
 * form for these ops: a call that mncclAlgoAuto or a forced mncclAlgoOneShot would run one-shot runs
 * as a call the one-shot does not fit -- the read schedule where every rank can share its buffers,
 * else the ring -- and mncclCommInfo_t.last_algo reports what ran.
 *
 * Checks of ncclRedOpCreatePreMulSum, in this order: NULL comm, op or scalar: ncclInvalidArgument;
 * an unsupported datatype: ncclInternalError; the communicator's sticky error is returned;
 * ncclScalarDevice (or any other residence): ncclInvalidUsage; a 17th live op: ncclInvalidUsage.
 * ncclRedOpDestroy: NULL comm: ncclInvalidArgument; a built-in or unknown handle: ncclInvalidArgument.
 * In a collective: ops 0 - 4 are checked as before, before the communicator is read; a value from
 * MNCCL_FIRST_USER_OP up is looked up in the communicator: an unknown handle is ncclInternalError
 * like any unsupported op, a handle created for another datatype ncclInvalidArgument, nothing
 * launched or negotiated.  No exception crosses the boundary. */
typedef enum { ncclScalarDevice = 0, ncclScalarHostImmediate = 1 } ncclScalarResidence_t;
#define MNCCL_FIRST_USER_OP 5
ncclResult_t ncclRedOpCreatePreMulSum(ncclRedOp_t* op, void* scalar, ncclDataType_t datatype,
                                      ncclScalarResidence_t residence, ncclComm_t comm);
ncclResult_t ncclRedOpDestroy(ncclRedOp_t op, ncclComm_t comm);

/* fp8 (NCCL's and RCCL's ncclFloat8e4m3 = 10 / ncclFloat8e5m2 = 11; detected by the symbol
 * mncclDataTypeSize and its answer for the two values, MNCCL_VERSION stays 600).  Every call accepts
 * the two types wherever it accepts ncclBfloat16, with the same checks in the same order: the calls
 * that fold (ncclAllReduce, ncclReduceScatter, ncclReduce with ncclSum / ncclProd / ncclMax / ncclMin
 * and ncclRedOpCreatePreMulSum ops; mncclLocalReduce with the four built-in ops), the calls that only
 * move bytes, with element size 1 (ncclAllGather, ncclBroadcast, ncclAllToAll, ncclAllToAllv,
 * ncclGather, ncclScatter, ncclSend, ncclRecv), and ncclRedOpCreatePreMulSum, whose scalar is one fp8
 * byte.  ncclAvg stays ncclInternalError.  Every schedule and form the 16-bit types have works: ring,
 * read, one-shot, grid form, registered windows, HIP-graph capture, one rank, host buffers.
 *
 * Encodings: both OCP (not MI300's fnuz).  E4M3 is e4m3fn: bias 7, no infinities, NaN 0x7f / 0xff,
 * largest finite value 448.  E5M2: bias 15, IEEE-like, 0x7c / 0xfc are +-inf, 0x7d..0x7f / 0xfd..0xff
 * NaN, largest finite value 57344.
 *
 * Result, bit for bit (ncclBfloat16's rule: widen exactly, operate in float, round once).  ncclSum,
 * ncclProd: r = float(a) op float(b), one IEEE single-precision operation (the product of two fp8
 * values is exact), then encode(r).  ncclMax, ncclMin: the decoded values are compared and an
 * operand's byte is returned unchanged -- (fa > fb) ? a : b and (fa < fb) ? a : b, with a the local
 * element and b the incoming one (op(x_q, acc)); what happens to NaN and +-0 follows from that
 * expression.  encode(r): NaN gives a NaN of the type (which one is unspecified); +-inf gives +-inf
 * for E5M2 (it cannot arise for E4M3); a finite r is rounded to nearest even onto the type's finite
 * grid, subnormals included; a finite r that rounds beyond the largest finite value SATURATES to
 * +-448 / +-57344 and never becomes inf or NaN; the sign of zero is r's.  A pre-multiplied sum:
 * y = encode(float(s) * float(x)), one product and one rounding, and the y are summed as ncclSum sums
 * them -- two roundings, no fusion, ncclAllReduce's tail unscaled, as for every datatype.  The
 * association across ranks is unchanged -- chunk c: acc = x_c, then acc = op(x_q, acc) for
 * q = c+1 ... c-1 -- re-encoded to fp8 after every step, so every schedule gives the same bits.
 *
 * 16-byte vectors.  The vector path's rule is unchanged: pointers dword-aligned and chunk bytes a
 * multiple of 4.  A one-byte type misses it for three chunk lengths out of four and then runs the
 * element path (same bits, one element per access): callers who care keep counts per rank a
 * multiple of 4.
 *
 * mncclDataTypeSize writes the element size of a supported datatype to *size and returns ncclSuccess;
 * an unsupported datatype is ncclInvalidArgument with *size untouched, a NULL size
 * ncclInvalidArgument. */
#define ncclFloat8e4m3 ((ncclDataType_t)10)
#define ncclFloat8e5m2 ((ncclDataType_t)11)
ncclResult_t mncclDataTypeSize(ncclDataType_t datatype, size_t* size);

/* Sub-communicators (NCCL's ncclCommSplit: name, argument order and meaning; detected by the symbol,
 * MNCCL_VERSION stays 600 and mncclCommInfo_t does not grow).  COLLECTIVE over every rank of `comm`.
 * Ranks passing the same color >= 0 form one new communicator; within it the ranks are ordered by
 * `key`, ascending -- keys may be negative or equal, and ties are broken by the rank in `comm`.  A
 * rank passing NCCL_SPLIT_NOCOLOR takes part in the exchange and gets *newcomm = NULL with
 * ncclSuccess.  A group of one is a valid one-rank communicator, and a child may be split again.  So
 * tensor- / data- / pipeline-parallel groups come from one ncclCommInitRank: no second port, no
 * MINI_NCCL_PORT changed between two calls, no rank numbering worked out by the caller.
 *
 * Checks, in this order (no exception crosses the boundary):
 *  1. a NULL comm or a NULL newcomm: ncclInvalidArgument;
 *  2. a group is open on this thread: ncclInvalidUsage, the group stays open and clean;
 *  3. a non-NULL config: ncclInvalidUsage (ncclConfig_t is opaque here: the child takes its parent's
 *     configuration);
 *  4. color < 0 other than NCCL_SPLIT_NOCOLOR: ncclInvalidArgument;
 *  5. with the communicator: its sticky error is returned;
 *  6. the exchange: any failure -- a peer gone, the bootstrap timeout
 *     MINI_NCCL_BOOTSTRAP_TIMEOUT_MS, a child that cannot be built -- is ncclSystemError on every rank
 *     that sees it.
 * Checks 1 - 4 happen before the communicator is read or any peer is contacted and leave *newcomm
 * untouched; as in NCCL their arguments are the caller's to keep valid on EVERY rank (a rank refused
 * there does not join the exchange the others wait in).  In 5 and 6 *newcomm is NULL on return and
 * the parent stays usable.
 *
 * The call first waits on the host for the parent's previous call, as mncclCommRegister does: no
 * collective of the parent is in flight while sockets are exchanged.  The exchange is two rounds
 * over the parent's bootstrap connections -- every rank's (color, key), then the ephemeral loopback
 * port each group's new rank 0 already listens on -- so no well-known port is used.
 *
 * A child is a full, independent communicator: its own scratch and mailbox, counters, control page,
 * read-schedule board, registered windows, user-created ops, sticky error, last_algo and bootstrap
 * connections (led by its new rank 0).  From the parent it takes the configuration BY COPY -- the
 * environment is not read again, and its schedule starts at the configured MINI_NCCL_ALGO, not at a
 * later mncclCommSetAlgo of the parent -- and the parent's GPU (the call makes that device current
 * while it builds the child and restores the caller's).  It does NOT inherit registered windows or
 * ncclRedOpCreatePreMulSum handles: a parent's handle used on the child is an unknown handle,
 * ncclInternalError.  Every collective, ncclSend / ncclRecv, windows and ops work on a child as on
 * any communicator.  Parent and children may be destroyed in any order (each ncclCommDestroy is
 * collective over that communicator's own ranks); a child keeps working after its parent is gone.
 *
 * Residency: sibling groups run their kernels on the same GPUs at the same time, so a child's
 * mncclCommInfo_t.run_pipelines is capped for the whole family -- by the ranks its parent (and,
 * through it, the first ancestor) counted on the most crowded GPU -- and never exceeds its
 * parent's; ranks_on_device stays the child's own count.
 *
 * Concurrency is NCCL's rule: calls on two communicators of one process -- a parent and a child, or
 * two children -- may overlap only if EVERY rank issues them in the same order.  Overlapping calls on
 * a parent and its child are also not covered by the residency cap above. */
#define NCCL_SPLIT_NOCOLOR (-1)
typedef struct ncclConfig ncclConfig_t; /* opaque; only NULL is accepted */
ncclResult_t ncclCommSplit(ncclComm_t comm, int color, int key, ncclComm_t* newcomm, ncclConfig_t* config);

ncclResult_t mncclLocalReduce(void* out, const void* local, const void* incoming, size_t count,
                              ncclDataType_t datatype, ncclRedOp_t op, hipStream_t stream);

ncclResult_t mncclCommGetAsyncError(ncclComm_t comm, ncclResult_t* asyncError);

ncclResult_t mncclCommGetInfo(ncclComm_t comm, mncclCommInfo_t* info);
/* mncclCommGetInfo writes the pre-300 prefix only (up to ipc_open_failures), so a caller built
   against an older header is never overrun; mncclCommGetInfoV writes min(size,
   sizeof(mncclCommInfo_t)) bytes: callers pass their struct's size */
ncclResult_t mncclCommGetInfoV(ncclComm_t comm, void* info, size_t size);

/* every rank must make the same choice before its next all-reduce; mncclAlgoAuto restores the
   default; mncclAlgoDirect -> ncclInvalidArgument (removed in 400) */
ncclResult_t mncclCommSetAlgo(ncclComm_t comm, int algo);

/* Collective diagnostic: every rank streams `bytes` (0 = its whole scratch region) into the
 * next rank's scratch (allPeers bit 0 = 0: one xGMI link per rank, the ring's) or into every
 * peer's at once (bit 0 = 1: the mesh, the read schedule's), `iters` times, with the hot
 * path's store form; *gbps = bytes per second per destination link.  Further bits of allPeers
 * select variants for comparison: bits 1-2 = the remote accesses' cache policy (0 = the hot
 * path's sc0 sc1, 1 = non-temporal, 2 = default), bit 3 = pull (load from the peers' scratch
 * over the link instead of storing into it), bit 4 = the peers' ordinary device memory (a
 * hipMalloc buffer each rank exports for the probe -- what the read schedule loads from)
 * instead of their uncached scratch.  Call only when no all-reduce is in flight on any rank (it
 * overwrites scratch slots). */
ncclResult_t mncclCommLinkProbe(ncclComm_t comm, int allPeers, size_t bytes, int iters, double* gbps);

/* Registered windows (since 500; NCCL's collective buffer registration; since 600 the no-rendezvous
 * launch below applies when no two ranks share a GPU or with MINI_NCCL_WINDOW_RENDEZVOUS=0 --
 * otherwise window calls are negotiated like any other, same results).  COLLECTIVE: every rank
 * calls mncclCommRegister with its buffer of the window -- device memory of its own GPU, the same
 * `size` on every rank -- in the same order (the window's number is the registration's).  After
 * it, an ncclAllReduce whose send and recv lie in registered windows -- the SAME windows at the
 * SAME byte offsets on every rank, with the same count / datatype / op (the symmetric layout of a
 * data-parallel gradient buffer) -- runs the read schedule with no host rendezvous: the call only
 * publishes its record and launches, so with MINI_NCCL_BLOCKING=0 a rank returns without waiting
 * for its peers.  The promise is checked on the device before any peer buffer is touched; a call
 * that breaks it (other windows or offsets on some rank, or an unregistered buffer where a peer
 * passed a registered one) fails with ncclInvalidUsage on every rank and the communicator is no
 * longer usable.  The buffer must stay allocated until mncclCommDeregister (also collective, same
 * order); calls on buffers outside any window are negotiated per call as before.  *handle
 * identifies the window; a communicator of one rank accepts and ignores windows. */
ncclResult_t mncclCommRegister(ncclComm_t comm, void* buff, size_t size, void** handle);
ncclResult_t mncclCommDeregister(ncclComm_t comm, void* handle);

/* library version, 10000*major + 100*minor + patch */
int mncclVersion(void);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* MINI_NCCL_EXT_H_ */
