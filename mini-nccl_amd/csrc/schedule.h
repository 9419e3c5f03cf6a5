// schedule.h -- the per-channel message schedules, shared verbatim by the HIP kernels
// (kernels.hip) and by the host-side schedule simulator (sim.cpp, run by the CPU test
// suite), so the index math the GPU executes is the index math the CPU tests check.
//
// Ring (reference mini_nccl.cu:108-194).  The reference walks step-major: for each step,
// every slice of the chunk.  Each element's arithmetic depends only on which chunk it
// is in, so we walk slice-major per channel instead (for each slice owned by the
// channel, all 2(n-1) steps), which keeps every link busy with a 2-slot FIFO and gives
// per element exactly the reference's sequence of ops:
//   op 0         : send the raw chunk r                         (SR step 0 send, :128-131)
//   op 1..n-1    : SR step i = op-1 receives chunk (r-i-1) mod n (:110) and reduces
//                  op(local, incoming) (:126); i < n-2 forwards the partial (the next
//                  step's send of the same chunk, :109), i == n-2 is the final value of
//                  chunk r+1: stored to recv AND forwarded (all-gather step 0, :160)
//   op n..2n-2   : AG step j = op-n receives chunk (r-j) mod n (:172, the sender's
//                  send_idx (r-1)-j+1), stores it to recv, forwards unless j == n-2.
// Messages per channel iteration: 2(n-1) sent to r+1, 2(n-1) received from r-1.
//
// Read (the default for device buffers, same fold order, every link): rank r folds slice s of
// its own chunk r straight from the peers' send buffers in ring order r, r+1, ..., r-1
// (acc = op(x_q, acc): the visited rank's value is the LEFT/local operand exactly as at rank q
// of the ring) and pushes the result into every peer's recv (kernels.hip read_kernel).
//
// The two halves (ncclReduceScatter / ncclAllGather): the read schedule's fold without the pushes,
// its pushes without a fold (kernels.hip scatter_fold / gather_push), and the ring's two phases as
// op tables of their own (coll_op below).
//
// One-shot (small calls the read schedule cannot take): every rank stores its pieces into every
// peer's scratch and folds each piece of the result from all n ranks in that same order
// (kernels.hip oneshot_kernel; geometry below).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MNCCL_HD __host__ __device__ __forceinline__
#else
#define MNCCL_HD inline
#endif

namespace mnccl {

enum RingKind : int {
  kSend = 0,            // out <- local
  kReduceSend = 1,      // out <- op(local, in)
  kReduceCopySend = 2,  // v = op(local, in); recv <- v; out <- v
  kCopySend = 3,        // recv <- in; out <- in
  kCopy = 4,            // recv <- in
  // the rooted reduce's ring on the ranks that are not the root: the all-reduce's second phase
  // with its stores into recv masked off (coll_op)
  kForward = 5,         // out <- in
  kDrop = 6             // the message is received and dropped
};

struct RingOp {
  int kind;
  int chunk;     // chunk index the op touches
  int send_msg;  // message index (within the iteration) sent to r+1, or -1
  int recv_msg;  // message index received from r-1, or -1
};

// Threads per workgroup of the persistent kernels (MINI_NCCL_THREADS is clamped to it): the
// launch bound lets the compiler give a pipeline's wave up to 512 VGPRs instead of the 128 a
// 1024-thread bound allows (the direct fold spilled at 128); one wave per workgroup is the default.
constexpr int kMaxThreads = 256;
// Largest message payload / slot stride (MINI_NCCL_SLICE_SIZE is clamped to it): message
// lengths and slot offsets are 32-bit in the kernels' buffer resources.
constexpr uint64_t kMaxSlice = 256ull << 20;
// Default pipelines of the persistent kernels: one per CU of the 256.
constexpr int kDefaultPipelines = 256;

MNCCL_HD int mod_n(int a, int n) { return ((a % n) + n) % n; }

MNCCL_HD int ring_num_ops(int n) { return 2 * n - 1; }
MNCCL_HD int ring_msgs_per_iter(int n) { return 2 * (n - 1); }

MNCCL_HD RingOp ring_op(int n, int r, int k) {
  RingOp o;
  if (k == 0) {
    o.kind = kSend; o.chunk = r; o.send_msg = 0; o.recv_msg = -1;
  } else if (k < n) {
    const int i = k - 1;
    o.kind = (i < n - 2) ? kReduceSend : kReduceCopySend;
    o.chunk = mod_n(r - i - 1, n);
    o.send_msg = k; o.recv_msg = k - 1;
  } else {
    const int j = k - n;
    o.kind = (j < n - 2) ? kCopySend : kCopy;
    o.chunk = mod_n(r - j, n);
    o.send_msg = (j < n - 2) ? k : -1;
    o.recv_msg = k - 1;
  }
  return o;
}

// The ring's two halves as collectives of their own (ncclReduceScatter / ncclAllGather on the
// fallback path; ring_kernel picks the table by CollParams::coll at run time).  coll 0 is the
// all-reduce above, unchanged.
//   Reduce-scatter (n + 1 ops, n messages per iteration and link): chunk c starts at rank c, is
//   folded as op(local, incoming) at c+1, ..., c-1 -- the all-reduce's association -- and is then
//   handed one more hop to its owner c, whose recv holds only that chunk (the host passes
//   recv - r * chunk_bytes, so the index math stays the all-reduce's):
//     op 0       : send the raw chunk r
//     op 1..n-1  : receive chunk (r-k) mod n, reduce, forward
//     op n       : receive the finished chunk r, store it
//   All-gather (n ops, n - 1 messages): the all-reduce's second phase starting from the raw chunk
//   (the host passes send - r * chunk_bytes; the own chunk reaches the own recv by a device copy
//   before the launch when the call is not in place):
//     op 0       : send chunk r
//     op 1..n-2  : receive chunk (r-k) mod n, store, forward
//     op n-1     : receive chunk (r+1) mod n, store
//
// The two rooted collectives (ncclBroadcast / ncclReduce; `root` is rank-uniform).  Their chunks
// are q = ceil(count / n) elements, the trailing ones short or empty (rooted_len): no tail.
//   Broadcast (1 op, 1 message per iteration on every link but root-1 -> root, which carries
//   nothing: each link's counters advance by what it carried, coll_tx_msgs / coll_rx_msgs, so
//   sender and receiver of every link agree): the whole buffer is ONE chunk, slice-pipelined down
//   the chain root -> root+1 -> ... -> root-1:
//     root              : send
//     the ranks between : receive, store, forward
//     root-1            : receive, store
//   Reduce (the all-reduce's 2n - 1 ops and 2(n-1) messages): the all-reduce's table, on every rank
//   but the root with the stores into recv masked off -- kReduceCopySend becomes kReduceSend,
//   kCopySend kForward, kCopy kDrop -- so the root's recv has the all-reduce's association by
//   construction and nobody else's recv is touched.
//
// The all-to-all (ncclAllToAll: block q of rank r's send becomes block r of rank q's recv; a chunk
// is one block of `count` elements and both buffers hold n of them).  On the ring the block from
// rank s to rank s + d travels d hops, so per iteration, for d = 1 .. n-1 in this order, with
// m_d = d(d-1)/2 the group's first message:
//     kSend     of send block (r+d) mod n, send_msg m_d
//     kForward  j = 1 .. d-1: recv_msg m_d + j - 1, send_msg m_d + j
//     kCopy     into recv block (r-d) mod n, recv_msg m_d + d - 1
// (n-1)(n+2)/2 ops and n(n-1)/2 messages per iteration on every link; every message is received by
// the op right after the one that sent it on the rank before, as in the tables above.  Each op
// touches only one of send and recv, so one `chunk` per op is enough.  The own block reaches the
// own recv by a device copy before the launch, as the ring's all-gather gets its own chunk.
//
// The variable all-to-all (ncclAllToAllv, kCollAllToAllV) has no ring table of its own: off the read
// schedule it runs the table above on blocks padded to the largest one (Comm::all_to_all_v).
//
// The halves with per-rank counts (mncclAllGatherv / mncclReduceScatterv, kCollAllGatherV /
// kCollReduceScatterV) have none either: off the read schedule they run the two tables above on
// blocks padded to the largest one (Comm::vhalf).
//
// Gather and scatter (ncclGather / ncclScatter; a chunk is one block of `count` elements, the root's
// large buffer holds n of them; `root` is rank-uniform).  Both are a chain in ring direction, with
// pos = (r - root) mod n the rank's place in it; the op count and each link's message count depend
// on pos, and each link's counters advance by what it carried (coll_tx_msgs / coll_rx_msgs).
//   Gather (blocks travel towards the root, which sits at the chain's end; the link root -> root+1
//   carries nothing; the host passes send - r * chunk_bytes, as for the all-gather):
//     pos p >= 1 : kSend of the own block as message 0, then kForward of messages 0 .. p-2 from
//                  behind, sent on as messages 1 .. p-1 (p ops, p messages sent, p - 1 received)
//     the root   : kCopy of messages 0 .. n-2 into the blocks of the ranks at pos n-1, n-2, .., 1
//   Scatter (blocks travel away from the root; the link root-1 -> root carries nothing; the host
//   passes recv - r * chunk_bytes, as for the reduce-scatter):
//     the root   : kSend of the blocks for pos n-1, .., 1 as messages 0 .. n-2
//     pos p >= 1 : kForward of messages 0 .. n-p-2, then kCopy of message n-p-1 into its recv
//                  (n - p ops and messages received, n - p - 1 sent)
//   The root's own block reaches its place by a device copy before the launch when the call is not
//   in place, as the ring's all-gather gets its own chunk.
enum Coll : int {
  kCollAllReduce = 0, kCollReduceScatter = 1, kCollAllGather = 2, kCollBroadcast = 3, kCollReduce = 4, kCollAllToAll = 5,
  kCollAllToAllV = 6, kCollGather = 7, kCollScatter = 8,
  // the halves with per-rank counts (mncclAllGatherv / mncclReduceScatterv): like kCollAllToAllV they
  // have no ring table of their own -- off the read schedule they run the ring's halves on blocks
  // padded to the largest one (Comm::vhalf)
  kCollAllGatherV = 9, kCollReduceScatterV = 10
};

// r, root: gather and scatter only (their op count depends on the rank's place in the chain; the
// defaults give the root's, the largest)
MNCCL_HD int coll_num_ops(int coll, int n, int r = 0, int root = 0) {
  if (coll == kCollGather) return r == root ? n - 1 : mod_n(r - root, n);
  if (coll == kCollScatter) return r == root ? n - 1 : n - mod_n(r - root, n);
  return coll == kCollReduceScatter ? n + 1
         : coll == kCollAllGather   ? n
         : coll == kCollBroadcast   ? 1
         : coll == kCollAllToAll    ? (n - 1) * (n + 2) / 2
                                    : ring_num_ops(n);
}
// messages per iteration on a link that carries the collective (Broadcast: all but root-1 -> root)
MNCCL_HD int coll_msgs_per_iter(int coll, int n) {
  return coll == kCollReduceScatter ? n
         : coll == kCollAllGather   ? n - 1
         : coll == kCollBroadcast   ? 1
         : coll == kCollAllToAll    ? n * (n - 1) / 2
                                    : ring_msgs_per_iter(n);
}
// messages per iteration rank r sends to r+1 / receives from r-1: what its counters advance by
// (gather and scatter: a link carries as many blocks as lie behind it in the chain)
MNCCL_HD int coll_tx_msgs(int coll, int n, int r, int root) {
  if (coll == kCollGather) return mod_n(r - root, n);
  if (coll == kCollScatter) return n - 1 - mod_n(r - root, n);
  return coll == kCollBroadcast && mod_n(r - root, n) == n - 1 ? 0 : coll_msgs_per_iter(coll, n);
}
MNCCL_HD int coll_rx_msgs(int coll, int n, int r, int root) {
  if (coll == kCollGather) return r == root ? n - 1 : mod_n(r - root, n) - 1;
  if (coll == kCollScatter) return r == root ? 0 : n - mod_n(r - root, n);
  return coll == kCollBroadcast && r == root ? 0 : coll_msgs_per_iter(coll, n);
}
MNCCL_HD RingOp coll_op(int coll, int n, int r, int k, int root = 0) {
  RingOp o;
  if (coll == kCollGather) {
    const int pos = mod_n(r - root, n);
    if (pos == 0) {  // message k is the block of the rank at pos n-1-k
      o.kind = kCopy; o.chunk = mod_n(root + n - 1 - k, n); o.send_msg = -1; o.recv_msg = k;
    } else {
      o.kind = k == 0 ? kSend : kForward; o.chunk = r; o.send_msg = k; o.recv_msg = k - 1;  // (k == 0: -1)
    }
    return o;
  }
  if (coll == kCollScatter) {
    const int pos = mod_n(r - root, n);
    if (pos == 0) {  // message k is the block for the rank at pos n-1-k
      o.kind = kSend; o.chunk = mod_n(root + n - 1 - k, n); o.send_msg = k; o.recv_msg = -1;
    } else {
      const bool last = k == n - pos - 1;
      o.kind = last ? kCopy : kForward; o.chunk = r; o.send_msg = last ? -1 : k; o.recv_msg = k;
    }
    return o;
  }
  if (coll == kCollBroadcast) {
    const int pos = mod_n(r - root, n);  // place in the chain
    o.kind = pos == 0 ? kSend : pos < n - 1 ? kCopySend : kCopy;
    o.chunk = 0;
    o.send_msg = pos < n - 1 ? 0 : -1;
    o.recv_msg = pos > 0 ? 0 : -1;
    return o;
  }
  if (coll == kCollReduce) {
    o = ring_op(n, r, k);
    if (r != root)
      o.kind = o.kind == kReduceCopySend ? kReduceSend : o.kind == kCopySend ? kForward : o.kind == kCopy ? kDrop : o.kind;
    return o;
  }
  if (coll == kCollAllToAll) {
    // group d holds d + 1 ops and starts at op (d-1)(d+2)/2; j: the op's place in its group
    int d = 1, j = k;
    while (j > d) j -= d + 1, ++d;
    const int m = d * (d - 1) / 2;
    o.kind = j == 0 ? kSend : j < d ? kForward : kCopy;
    o.chunk = j == 0 ? mod_n(r + d, n) : j < d ? 0 : mod_n(r - d, n);
    o.send_msg = j < d ? m + j : -1;
    o.recv_msg = j > 0 ? m + j - 1 : -1;
    return o;
  }
  if (coll != kCollReduceScatter && coll != kCollAllGather) return ring_op(n, r, k);
  const int last = coll_num_ops(coll, n) - 1;
  if (k == 0) {
    o.kind = kSend; o.chunk = r; o.send_msg = 0; o.recv_msg = -1;
  } else if (k < last) {
    o.kind = coll == kCollReduceScatter ? kReduceSend : kCopySend;
    o.chunk = mod_n(r - k, n);
    o.send_msg = k; o.recv_msg = k - 1;
  } else {
    o.kind = kCopy;
    o.chunk = coll == kCollReduceScatter ? r : mod_n(r + 1, n);
    o.send_msg = -1; o.recv_msg = k - 1;
  }
  return o;
}

// Peer order of the read schedule's fold (ring order from r + 1) and of its pushes.
MNCCL_HD int direct_peer(int n, int r, int k) { return mod_n(r + k, n); }  // k = 1..n-1

// Read schedule (MINI_NCCL_ALGO=read): no scratch; rank r loads the peers' raw slices of chunk
// r straight from their send buffers and stores the result into every rank's recv.  Messages per
// (pair, pipeline) and call, all on the READY word: START and DONE; the count advances by
// iters + 2 (the 4.0-5.x load form also sent one READY per iteration; every rank counts alike).
MNCCL_HD uint64_t read_msgs_per_call(uint32_t iters) { return (uint64_t)iters + 2; }

// Pipelines a call runs (ring and read alike): one per slice, up to all C of them, rounded up to
// whole workgroups of `waves` pipelines.  The others sit the call out on every rank alike (a
// pure function of the call's size and the rank-uniform geometry), so their per-pair counters
// stay in step; a small call then dispatches, handshakes and drains a few waves, not C (the
// reference moves only the slices that exist, mini_nccl.cu:112-115).  Slice s of a call goes
// to pipeline s mod A (iteration s / A).
MNCCL_HD int call_pipelines(uint64_t nslices, int C, int waves) {
  uint64_t a = nslices < (uint64_t)C ? nslices : (uint64_t)C;
  if (a == 0) a = 1;
  a = (a + (uint64_t)waves - 1) / (uint64_t)waves * (uint64_t)waves;
  return a < (uint64_t)C ? (int)a : C;
}

// Slice geometry shared by both schedules: pipeline w of a call running A pipelines owns slices
// w, w+A, w+2A, ... of every chunk; message bytes of slice s (0 for the padding slices past the end, which
// still move flags so every channel sends the same number of messages).
MNCCL_HD uint64_t slice_len(uint64_t chunk_bytes, uint64_t slice_bytes, uint64_t s) {
  const uint64_t off = s * slice_bytes;
  if (off >= chunk_bytes) return 0;
  const uint64_t rest = chunk_bytes - off;
  return rest < slice_bytes ? rest : slice_bytes;
}

// ncclAllToAllv on the read schedule (kernels.hip varblock_push): the call's slices are cut for the
// LARGEST block of the whole matrix, and slice s of the block for one destination covers the bytes
// [s * slice_bytes, s * slice_bytes + varblock_len) of that block -- 0 once the block is exhausted,
// and for empty blocks.  varblock_len_at: the same from the slice's byte offset (what the kernel has).
MNCCL_HD uint64_t varblock_len_at(uint64_t block_bytes, uint64_t slice_bytes, uint64_t off) {
  if (off >= block_bytes) return 0;
  const uint64_t rest = block_bytes - off;
  return rest < slice_bytes ? rest : slice_bytes;
}
MNCCL_HD uint64_t varblock_len(uint64_t block_bytes, uint64_t slice_bytes, uint64_t s) {
  return varblock_len_at(block_bytes, slice_bytes, s * slice_bytes);
}

// mncclReduceScatterv / mncclAllGatherv on the read schedule (kernels.hip vhalf_fold / vhalf_push):
// the call's slices are cut for the LARGEST block of the call, M = max(counts) * element size (the
// same on every rank), and rank r's slice s covers the bytes [base_r + s * slice_bytes, + vhalf_len)
// of the array-side buffers, base_r = displs[r] * element size -- 0 once rank r's own block of
// `block_bytes` has run out, and for an empty block: such a slice touches nothing, and the rank
// still exchanges START and DONE.
MNCCL_HD uint64_t vhalf_len(uint64_t block_bytes, uint64_t slice_bytes, uint64_t s) {
  const uint64_t off = s * slice_bytes;
  if (off >= block_bytes) return 0;
  const uint64_t rest = block_bytes - off;
  return rest < slice_bytes ? rest : slice_bytes;
}

// The rooted collectives' slices (ncclBroadcast / ncclReduce): the buffer's `total_bytes` are cut
// into n chunks of chunk_bytes = ceil(count / n) elements, so the trailing chunks may be short or
// empty -- slice s of the chunk at byte `chunk_off` is additionally clamped to the buffer's end,
// and a slice at or past the end has length 0 and touches nothing.
MNCCL_HD uint64_t rooted_len(uint64_t total_bytes, uint64_t chunk_off, uint64_t chunk_bytes, uint64_t slice_bytes,
                             uint64_t s) {
  const uint64_t len = slice_len(chunk_bytes, slice_bytes, s), off = chunk_off + s * slice_bytes;
  if (off >= total_bytes) return 0;
  return len < total_bytes - off ? len : total_bytes - off;
}

// Payload bytes per message for one call: the configured slice for large chunks; for chunks
// too small to give every channel `depth` slices of it, ceil(chunk / (C * depth)) rounded up
// to whole waves of 16-byte vectors (1 KiB) and at least `min_slice` (kMinSlice), so small all-reduces
// still spread over every pipeline instead of queueing on a few.  A pure function of the
// call's size and the (rank-uniform) config: every rank picks the same value.  Scratch slot
// addresses keep the configured stride whatever the payload (scratch_slot_off), so calls of
// different sizes never alias each other's slots.  Slicing never changes results.
constexpr uint64_t kMinSlice = 1024;  // one 16-byte vector per lane of a wave
MNCCL_HD uint64_t effective_slice(uint64_t chunk_bytes, int C, uint64_t slice, uint64_t min_slice, int depth) {
  if (min_slice >= slice || depth < 1) return slice;
  const uint64_t per = (uint64_t)C * (uint64_t)depth;
  uint64_t want = (chunk_bytes + per - 1) / per;
  want = (want + 1023) & ~(uint64_t)1023;
  if (want < min_slice) want = min_slice;
  return want < slice ? want : slice;
}

// Read schedule payload: no scratch slot bounds it, so it aims for kReadDepth iterations per
// pipeline (a pipeline's first fold and last copy do not overlap anything: more, smaller
// iterations shrink that fill and drain) while slices stay >= kReadMinSlice; below that, fewer
// iterations of kReadMinSlice, down to the adaptive one-slice-per-pipeline payload of small
// calls.  Measured on the one-GPU proxy, 1 GiB per rank (profiles/r2_read_depth_sweep.txt):
// 4 ranks 508 -> 615 GB/s, 8 ranks 262 -> 301 GB/s, 2 ranks unchanged.  A pure function of the
// call's size and the rank-uniform config, like effective_slice.
constexpr int kReadDepth = 16;
constexpr uint64_t kReadMinSlice = 16u << 10;
MNCCL_HD uint64_t read_slice(uint64_t chunk_bytes, int C, uint64_t slice, uint64_t min_slice, int depth) {
  uint64_t s = effective_slice(chunk_bytes, C, slice, min_slice, depth);
  if (s < kReadMinSlice) {
    const uint64_t one = effective_slice(chunk_bytes, C, slice, min_slice, 1);
    s = one < kReadMinSlice ? one : kReadMinSlice;
  }
  return s;
}

// One-shot (kernels.hip oneshot_kernel): pipeline w = s * n + c carries slice s of chunk c --
// its message to every peer is that piece of this rank's send, and it folds that piece of the
// result from all n ranks' pieces.  A call takes it when its n x nslices pipelines fit one round
// (n x nslices <= C) and its bytes (n chunks) are at most kOneShotMaxBytes -- or at any size that
// fits when forced (MINI_NCCL_ALGO=oneshot).  Each rank sends (n - 1) x the call's bytes: a
// latency path, not a bandwidth one.  Under auto it replaces the ring for small calls whose
// buffers the read schedule cannot take (host memory, a full export table).
constexpr uint64_t kOneShotMaxBytes = 64u << 10;
MNCCL_HD uint64_t oneshot_slice(uint64_t chunk_bytes, int n, int C, uint64_t slot_bytes) {
  const int per = n > 0 && C / n > 0 ? C / n : 1;
  return effective_slice(chunk_bytes, per, slot_bytes, kMinSlice, 1);
}
MNCCL_HD bool oneshot_fits(uint64_t chunk_bytes, int n, int C, uint64_t slot_bytes, bool forced) {
  if (n < 2 || chunk_bytes == 0 || (!forced && chunk_bytes * (uint64_t)n > kOneShotMaxBytes)) return false;
  const uint64_t sl = oneshot_slice(chunk_bytes, n, C, slot_bytes);
  return sl <= slot_bytes && (chunk_bytes + sl - 1) / sl * (uint64_t)n <= (uint64_t)C;
}

// The read schedule's grid form (mncclAlgoReadGrid; kernels.hip read_grid_kernel): three launches
// instead of the persistent kernel -- a one-wave START, a grid of one-batch workgroups that only
// fold and push, a one-wave DONE -- with the protocol of a one-slice read call on pipeline 0.
// Chunks of at least kReadGridMin bytes (MINI_NCCL_GRID_MIN: a tuning knob, rank-uniform), whole
// 16-byte vectors, up to 8 ranks (the fold's peer groups); smaller or ragged calls run the
// persistent read kernel.  Measured in profiles/r4_read_grid_ab.txt and r5_grid_min_ab.txt (on the
// one-GPU proxy the grid form below 4 MiB chunks was slower or equal).
constexpr uint64_t kReadGridMin = 4ull << 20;
constexpr uint64_t kReadGridFloor = 64ull << 10;  // the smallest MINI_NCCL_GRID_MIN
MNCCL_HD bool read_grid_fits(uint64_t chunk_bytes, int n, uint64_t min_bytes = kReadGridMin) {
  return n >= 2 && n <= 8 && chunk_bytes >= min_bytes && chunk_bytes % 16 == 0;
}
// 16-byte vectors per lane in one grid workgroup (V KiB of the chunk, from every peer): one up to
// 4 ranks, two from 5 (profiles/r5_grid_v_ab.txt, 1 GiB per rank on the one-GPU proxy: 8 ranks
// 3.07 vs 4.72 ms per call with V = 2 vs 1 -- as fast as the persistent kernel -- while 2 and 4
// ranks are 7 % and 3 % faster with V = 1)
MNCCL_HD int read_grid_vectors(int n) { return n <= 4 ? 1 : 2; }

// Scratch layout: one region per PEER rank (n - 1 of them: the owner never sends to itself),
// [C][slots][slice_bytes] each.  region_index maps a peer rank q != owner to its region.
MNCCL_HD uint64_t scratch_region_bytes(int C, int slots, uint64_t slice_bytes) { return (uint64_t)C * slots * slice_bytes; }
MNCCL_HD int region_index(int owner, int q) { return q < owner ? q : q - 1; }
MNCCL_HD uint64_t scratch_slot_off(int C, int slots, uint64_t slice_bytes, int region, int w, uint64_t seq) {
  return (uint64_t)region * scratch_region_bytes(C, slots, slice_bytes) +
         ((uint64_t)w * slots + (seq % (uint64_t)slots)) * slice_bytes;
}

// Kernel geometry of one communicator (Comm, and the CPU tests through the simulator library):
// a pure function of the rank-uniform config and n, so every rank computes the same.
//  * workgroups: MINI_NCCL_CHANNELS if set; otherwise one pipeline per CU (256), bounded by the
//    reference's in-flight bound: WINDOW pending signalled requests, each covering SIGNAL_BATCH
//    messages (mini_nccl.cu:119,144,167), i.e. pipelines x slots <= WINDOW x SIGNAL_BATCH
//    messages in flight per link (64 x 16 = 1024 >= 256 x 2 at the defaults);
//  * then the scratch cap: (n-1) regions x pipelines x slots x slot <= cap (fewer pipelines, the
//    payload per message stays MINI_NCCL_SLICE_SIZE; only if one workgroup cannot fit does the
//    slot shrink, to whole KiB).
struct Geometry {
  int workgroups;
  int waves;             // per workgroup (threads / 64): pipelines = workgroups x waves
  uint64_t slot_bytes;   // slot stride and largest payload per message
  uint64_t scratch_bytes;
};
MNCCL_HD Geometry pipeline_geometry(int n, int channels, int threads, int window, int signal_batch, int slots,
                                    uint64_t slice, uint64_t cap) {
  Geometry g;
  g.waves = threads / 64 > 0 ? threads / 64 : 1;
  if (slots < 1) slots = 1;
  if (channels > 0) {
    g.workgroups = channels;
  } else {
    uint64_t inflight = (uint64_t)(window > 0 ? window : 1) * (uint64_t)(signal_batch > 0 ? signal_batch : 1);
    uint64_t P = inflight / (uint64_t)slots;
    if (P > (uint64_t)kDefaultPipelines) P = kDefaultPipelines;
    uint64_t wg = P / (uint64_t)g.waves;
    g.workgroups = wg < 1 ? 1 : (int)wg;
  }
  g.slot_bytes = slice;
  const uint64_t regions = n > 1 ? (uint64_t)(n - 1) : 0;
  if (regions) {
    const uint64_t per_wg = (uint64_t)g.waves * (uint64_t)slots * slice * regions;
    const uint64_t max_wg = cap / per_wg;
    if (max_wg < 1) {
      g.workgroups = 1;
      uint64_t s = (cap / ((uint64_t)g.waves * (uint64_t)slots * regions)) & ~(uint64_t)1023;
      g.slot_bytes = s < 1024 ? 1024 : s;
    } else if ((uint64_t)g.workgroups > max_wg) {
      g.workgroups = (int)max_wg;
    }
  }
  g.scratch_bytes = regions * scratch_region_bytes(g.workgroups * g.waves, slots, g.slot_bytes);
  return g;
}

// Mailbox layout (uint64 words, one 128-byte line per flag):
//   READY(src, w)  : written by rank src when its message for this rank landed
//   CREDIT(dst, w) : written by rank dst when it has consumed a message from this rank
//   ABORT          : written by any rank that gives up (timeout / host abort)
constexpr int kFlagStride = 16;  // uint64 words per flag line
MNCCL_HD uint64_t mbox_ready(int C, int src, int w) { return ((uint64_t)src * C + w) * kFlagStride; }
MNCCL_HD uint64_t mbox_credit(int n, int C, int dst, int w) { return ((uint64_t)n * C + (uint64_t)dst * C + w) * kFlagStride; }
MNCCL_HD uint64_t mbox_abort(int n, int C) { return (uint64_t)2 * n * C * kFlagStride; }
//   DEST(dst, w)   : behind ABORT, two lines per (receiving rank, pipeline): written by rank dst at
//                    the start of each point-to-point message it receives from this rank on a
//                    communicator with registered windows (kernels.hip p2p_window_group, p2p.h
//                    P2pDest) -- the record's three info words on the first line, then its tag, the
//                    pair's message counter + 1, on the second.  READY / CREDIT / ABORT keep their
//                    offsets.
constexpr int kDestInfoWords = 3;
MNCCL_HD uint64_t mbox_dest_info(int n, int C, int dst, int w) {
  return mbox_abort(n, C) + kFlagStride + ((uint64_t)dst * C + w) * 2 * kFlagStride;
}
MNCCL_HD uint64_t mbox_dest_tag(int n, int C, int dst, int w) { return mbox_dest_info(n, C, dst, w) + kFlagStride; }
MNCCL_HD uint64_t mbox_words(int n, int C) { return mbox_dest_info(n, C, n, 0); }

// Where message `seq` from rank `src` to rank `dst` (pipeline w) lives: in the receiver's
// scratch, region src -- the sender's stores cross the link.
MNCCL_HD uint64_t msg_slot_off(int C, int slots, uint64_t slot_bytes, int src, int dst, int w, uint64_t seq) {
  return scratch_slot_off(C, slots, slot_bytes, region_index(dst, src), w, seq);
}

// Topology rule of the default schedule (MINI_NCCL_ALGO=auto).  The read schedule loads from and
// pushes into every peer's memory directly, so it is only the fast path when every pair of GPUs
// is one xGMI hop apart -- an MI355X node's full mesh; over PCIe (or a multi-hop route) every
// byte would cross the host fabric and the ring, which moves 2(n-1)/n of the buffer through one
// neighbour link, is the safer choice.  Ranks sharing a GPU (the reference's perf_test topology)
// reach each other through that GPU's own memory: allowed.  A peer whose GPU this process cannot
// see cannot be classified: not allowed (the runtime could not tell us the link).  The reference
// decides per peer whether its same-host IPC path applies (RDMATransport.h:109-111,583-590);
// here every rank applies this to its own row and the communicator takes the AND over ranks
// (Comm::exchange_and_map), so every rank decides alike.  link[q * n + p] / hops[q * n + p]: how
// rank q's GPU reaches rank p's (kPeerSameGpu, kPeerUnknown, or the HSA link type: 2 PCIe, 4 xGMI).
enum : int { kPeerSameGpu = -1, kPeerUnknown = -2, kLinkPcie = 2, kLinkXgmi = 4 };
// 0: the read schedule may be the default; otherwise 1 + the first offending pair's index q * n + p
MNCCL_HD int topology_blocks_read(int n, const int* link, const int* hops) {
  for (int q = 0; q < n; ++q)
    for (int p = 0; p < n; ++p) {
      if (p == q) continue;
      const int l = link[q * n + p];
      if (l == kPeerSameGpu) continue;
      if (l != kLinkXgmi || hops[q * n + p] != 1) return 1 + q * n + p;
    }
  return 0;
}

// The pipelines a call may launch (Comm::run_pipes): pipeline w of every rank waits for pipeline w
// of its peers, so the waves a call launches on the most crowded GPU -- `most` ranks on a GPU of
// `cus` CUs, each CU's 4 SIMDs keeping `waves_per_simd` of the kernels' waves resident -- must all
// fit at once: min(P, cus x 4 x waves_per_simd / most), whole workgroups of `waves`, at least one.
// resident_cap: that budget alone, whole workgroups of `waves`, at least one.
MNCCL_HD int resident_cap(int waves, int cus, int most, int waves_per_simd) {
  if (most < 1) most = 1;
  if (waves < 1) waves = 1;
  int cap = cus * 4 * waves_per_simd / most / waves * waves;
  if (cap < waves) cap = waves;
  return cap;
}
MNCCL_HD int resident_pipes(int P, int waves, int cus, int most, int waves_per_simd) {
  const int cap = resident_cap(waves, cus, most, waves_per_simd);
  return P < cap ? P : cap;
}

// Point-to-point (ncclSend / ncclRecv, kernels.hip p2p_kernel).  Both ends of a message must agree
// on its slices and pipelines without talking, so a message's geometry is a function of its byte
// count and the communicator's rank-uniform configuration only -- never of what else its group
// holds, nor of a pointer's alignment.
//  * p2p_pipes: the pipelines one message may use.  A launch gives every directed pair present in
//    its group one wave per pipeline, a rank can have 2 (n - 1) directed pairs busy at once, and all
//    of a launch's waves must be resident together on the most crowded GPU: the resident budget
//    (resident_cap for one-wave workgroups: the cap, not its minimum with the communicator's
//    pipelines) divided by 2 (n - 1), clamped to [1, C].  One rank: only the self pair exists.
//  * a message of `bytes` is cut into ceil(bytes / slot_bytes) slices, slice s of slice_len(bytes,
//    slot_bytes, s) bytes; it uses pipelines 0 .. A - 1, A = min(p2p_pipes, nslices), and pipeline w
//    carries slices w, w + A, ..., one message each on the pair's own READY / CREDIT / slot /
//    counter entries (mbox_ready, mbox_credit, msg_slot_off, tx_seq / rx_seq at [peer * C + w]).
MNCCL_HD int p2p_pipes(int n, int C, int cus, int most, int waves_per_simd) {
  if (C < 1) C = 1;
  if (n < 2) return 1;
  const int per = resident_cap(1, cus, most, waves_per_simd) / (2 * (n - 1));
  return per < 1 ? 1 : per < C ? per : C;
}
MNCCL_HD uint64_t p2p_nslices(uint64_t bytes, uint64_t slot_bytes) { return (bytes + slot_bytes - 1) / slot_bytes; }
MNCCL_HD int p2p_msg_pipes(uint64_t bytes, uint64_t slot_bytes, int pipes) {
  const uint64_t ns = p2p_nslices(bytes, slot_bytes);
  return ns < (uint64_t)pipes ? (int)ns : pipes;
}
// slices pipeline w of a message carries: what the pair's counters on w advance by
MNCCL_HD uint64_t p2p_pipe_msgs(uint64_t bytes, uint64_t slot_bytes, int pipes, int w) {
  const uint64_t ns = p2p_nslices(bytes, slot_bytes);
  const uint64_t A = (uint64_t)p2p_msg_pipes(bytes, slot_bytes, pipes);
  return (uint64_t)w < A ? (ns - (uint64_t)w + A - 1) / A : 0;
}

// Whether a read-schedule call launches in the grid form (kernels.hip read_start / read_grid /
// read_done) rather than the persistent read_kernel: forced (mncclAlgoReadGrid) or under auto,
// for the push form's calls that fit it.  Auto took the grid only with every rank on a GPU of its
// own until the grid's workgroup size followed the rank count (read_grid_vectors); since then it
// measured at least the persistent kernel's rate with co-located ranks too: 2 ranks 1.20x (the
// persistent kernel's bimodal placement), 4 ranks 1.04x, 8 ranks 0.99-1.02x
// (profiles/r5_read_vs_grid_forms.txt, r5_bench_n{2,8}_auto_grid.json).  Uniform across ranks:
// every input is.
MNCCL_HD bool read_grid_form(bool forced, bool auto_mode, bool vec, uint64_t chunk_bytes, int n,
                             uint64_t min_bytes = kReadGridMin) {
  return (forced || auto_mode) && vec && read_grid_fits(chunk_bytes, n, min_bytes);
}

// Kernel status bits (host-mapped status word)
// kStatusMismatch: a registered-window call whose ranks passed different windows / offsets / count /
// dtype / op (the START signatures differ, read_kernel): no data was touched, the call fails with
// ncclInvalidUsage on every rank.
enum : uint32_t { kStatusTimeout = 1u, kStatusHostAbort = 2u, kStatusRemoteAbort = 4u, kStatusMismatch = 8u };

// Word of a READY line (mbox_ready, 16 words per line) that carries the sender's call signature
// with its START of a registered-window call (0 = none).
constexpr int kSigWord = 1;

}  // namespace mnccl
