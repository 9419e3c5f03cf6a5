// sim.cpp -- host-side simulator of the ring / read / one-shot kernels' protocol, for the CPU test
// suite (no GPU).  Each (rank, channel) runs the same op sequence as kernels.hip, using the
// same schedule.h index math, scratch layout and mailbox layout; a wait that is not
// satisfied yields, and the scheduler round-robins over all programs.  It checks:
//   * the data each rank ends with (compared by the tests against oracle/ring_oracle.c),
//   * deadlock freedom for the given (n, channels, slots, sizes): no progress => -1,
//   * that the per-channel sequence bases carried across calls keep flags consistent.
// mnccl_sim_collective runs sequences of all-reduce / reduce-scatter / all-gather calls on one
// such state (the halves: schedule.h coll_op on the ring, kernels.hip scatter_fold / gather_push on
// the read schedule).  mnccl_sim_rooted adds ncclBroadcast / ncclReduce with a root per call (the
// ring's chain and masked ring, kernels.hip root_relay / root_fold), interleaved with the others.
// mnccl_sim_mixed adds ncclAllToAll (the ring's hop table, kernels.hip exchange_push) to those five.
// mnccl_sim_varblock adds ncclAllToAllv (kernels.hip varblock_push; the ring on padded blocks).
// mnccl_sim_all_collectives adds ncclGather / ncclScatter (the ring's chains, kernels.hip collect_push /
// deal_push) to those seven.
// mnccl_sim_vhalves adds mncclAllGatherv / mncclReduceScatterv (kernels.hip vhalf_push / vhalf_fold; the
// ring's halves on padded blocks) to the eight with uniform counts.
// mnccl_sim_p2p adds ncclSend / ncclRecv groups (kernels.hip p2p_kernel, one wave per (pair, pipeline)
// from p2p.h's argument builder), every rank running its own list of launches, between collectives.
// fp32 only (the schedule does not depend on the element type); ops as reference
// mini_nccl.cu:38-41 with a = local, b = incoming.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "p2p.h"
#include "schedule.h"
#include "vhalves.h"

using namespace mnccl;

namespace {

float apply(int op, float a, float b) {
  switch (op) {
    case 0: return a + b;
    case 1: return a * b;
    case 2: return (a > b) ? a : b;
    default: return (a < b) ? a : b;
  }
}

struct World {
  int n, C, K, op, algo;
  int coll = kCollAllReduce;  // the current call's collective (schedule.h Coll); for a half, the
                              // one-chunk buffer's pointer is shifted as Comm::launch shifts it
  std::vector<char> own;      // all-gather: per rank, whether the read kernel stores the own chunk
  int root = 0;               // the rooted collectives: the call's root and the buffer's bytes (their
  uint64_t total_bytes = 0;   // chunks are ceil(count / n) elements: schedule.h rooted_len)
  int A = 0;  // pipelines the current call runs (schedule.h call_pipelines)
  uint64_t slice, slot_bytes, chunk_bytes, nslices;  // payload per message, slot stride
  uint32_t iters;
  std::vector<const float*> send;
  std::vector<float*> recv;
  std::vector<float*> peer_recv;              // every rank's recv as its peers map it (CollParams::peer_recv: unshifted)
  std::vector<std::vector<char>> scratch;     // per rank
  std::vector<std::vector<uint64_t>> mbox;    // per rank
  std::vector<std::vector<uint64_t>> tx_seq, rx_seq;  // per rank: [peer * C + w]
  std::vector<uint64_t> sig;           // registered-window call: each rank's START signature (empty: none)
  std::vector<int> mismatch;           // per rank: pipelines that saw a differing signature
  // ncclAllToAllv (coll 6) on the read schedule: per (source r, destination q), at [r * n + q], the
  // block's bytes and its byte offsets in r's send and in q's recv (kernels.h VarBlockArgs)
  const uint64_t *vbytes = nullptr, *vsrc = nullptr, *vdst = nullptr;
  // mncclAllGatherv / mncclReduceScatterv (coll 9 / 10) on the read schedule: per rank, its block's byte
  // offset in every rank's array-side buffer and its length (kernels.h VHalfArgs)
  const uint64_t *hbase = nullptr, *hbytes = nullptr;

  // message `seq` from src to dst on pipeline w (schedule.h msg_slot_off: the receiver's scratch)
  char* slot(int src, int dst, int w, uint64_t seq) {
    return scratch[dst].data() + msg_slot_off(C, K, slot_bytes, src, dst, w, seq);
  }
  uint64_t& ready(int owner, int src, int w) { return mbox[owner][mbox_ready(C, src, w)]; }
  uint64_t& credit(int owner, int dst, int w) { return mbox[owner][mbox_credit(n, C, dst, w)]; }
};

// copy / reduce over `bytes` bytes of floats
void do_move(int kind, int op, const float* local, const float* in, float* recv, float* out, uint64_t bytes) {
  const uint64_t ne = bytes / 4;
  for (uint64_t i = 0; i < ne; ++i) {
    float v;
    switch (kind) {
      case kSend: v = local[i]; break;
      case kReduceSend:
      case kReduceCopySend: v = apply(op, local[i], in[i]); break;
      default: v = in[i]; break;
    }
    if (kind == kDrop) continue;
    if (kind == kReduceCopySend || kind == kCopySend || kind == kCopy) recv[i] = v;
    if (kind != kCopy) out[i] = v;
  }
}

struct Prog {
  int r, w;
  uint32_t it = 0;
  int k = 0;      // ring: op index within the iteration
  uint32_t j = 0; // read: stage
  bool done = false;
};

// One ring op (kernels.hip ring_kernel body); returns false if a wait is unsatisfied.
bool ring_step(World& W, Prog& P) {
  const int n = W.n, r = P.r, w = P.w, K = W.K;
  const int prev = mod_n(r - 1, n), next = mod_n(r + 1, n);
  const uint64_t tx_base = W.tx_seq[r][(size_t)next * W.C + w], rx_base = W.rx_seq[r][(size_t)prev * W.C + w];
  // each link's counters advance by what it carried (Broadcast's root-1 -> root: nothing)
  const int mpi_tx = coll_tx_msgs(W.coll, n, r, W.root), mpi_rx = coll_rx_msgs(W.coll, n, r, W.root);
  const uint64_t s = (uint64_t)P.it * W.A + w;  // slice s on pipeline s mod A (kernels.hip ring_kernel)
  const uint64_t soff = s * W.slice;
  const RingOp o = coll_op(W.coll, n, r, P.k, W.root);
  // ncclReduce: the message's length is clamped to the buffer's end for its chunk
  const uint64_t len = W.coll == kCollReduce
                           ? rooted_len(W.total_bytes, (uint64_t)o.chunk * W.chunk_bytes, W.chunk_bytes, W.slice, s)
                           : slice_len(W.chunk_bytes, W.slice, s);
  const uint64_t rseq = rx_base + (uint64_t)P.it * mpi_rx + (uint64_t)o.recv_msg,
                 sseq = tx_base + (uint64_t)P.it * mpi_tx + (uint64_t)o.send_msg;
  if (o.recv_msg >= 0 && W.ready(r, prev, w) < rseq + 1) return false;
  if (o.send_msg >= 0 && sseq + 1 > (uint64_t)K && W.credit(r, next, w) < sseq + 1 - K) return false;
  if (len) {
    const uint64_t coff = (uint64_t)o.chunk * W.chunk_bytes + soff;
    const float* local = (const float*)((const char*)W.send[r] + coff);
    float* recv = (float*)((char*)W.recv[r] + coff);
    const float* in = o.recv_msg >= 0 ? (const float*)W.slot(prev, r, w, rseq) : nullptr;
    float* out = o.send_msg >= 0 ? (float*)W.slot(r, next, w, sseq) : nullptr;
    do_move(o.kind, W.op, local, in, recv, out, len);
  }
  if (o.send_msg >= 0) W.ready(next, r, w) = sseq + 1;
  if (o.recv_msg >= 0) W.credit(prev, r, w) = rseq + 1;
  if (++P.k == coll_num_ops(W.coll, n, r, W.root)) {
    P.k = 0;
    if (++P.it == W.iters) P.done = true;
  }
  return true;
}

// One step of the read schedule (kernels.hip read_kernel): stage 0 publishes START, 1 waits for
// every peer's START, 2 runs the iterations, 3 publishes DONE (+ credits), 4 waits for every
// peer's DONE.  One step per iteration -- the fold of slice it of chunk r from the peers' send
// buffers, stored into this rank's recv AND pushed into every peer's recv at the same offset, no
// READY.  Every peer access touches the peer's own buffers (W.send / W.recv of that rank), so an
// in-place call whose order were wrong would read overwritten data and fail the oracle comparison.
bool read_step(World& W, Prog& P) {
  const int n = W.n, r = P.r, w = P.w;
  auto tx = [&](int d) { return W.tx_seq[r][(size_t)d * W.C + w]; };
  auto rx = [&](int q) { return W.rx_seq[r][(size_t)q * W.C + w]; };
  const uint64_t mpc = read_msgs_per_call(W.iters);
  const bool rooted = W.coll == kCollBroadcast || W.coll == kCollReduce;
  auto slice_bytes_of = [&](uint64_t s) {  // kernels.hip read_half<ROOTED>
    return rooted ? rooted_len(W.total_bytes, (uint64_t)r * W.chunk_bytes, W.chunk_bytes, W.slice, s)
                  : slice_len(W.chunk_bytes, W.slice, s);
  };
  auto fold = [&](uint32_t it) {  // slice `it` of chunk r, stored and pushed
    const uint64_t s = (uint64_t)it * W.A + w;
    const uint64_t len = slice_bytes_of(s);
    const uint64_t coff = (uint64_t)r * W.chunk_bytes + s * W.slice;
    const float* local = (const float*)((const char*)W.send[r] + coff);
    std::vector<float> res((size_t)(len / 4));
    for (uint64_t i = 0; i < len / 4; ++i) {
      float acc = local[i];
      for (int k = 1; k < n; ++k) {
        const int q = direct_peer(n, r, k);
        acc = apply(W.op, ((const float*)((const char*)W.send[q] + coff))[i], acc);
      }
      res[(size_t)i] = acc;
    }
    // every load of the slice came first (in place, recv chunk r of a peer is its send chunk r)
    if (len) {
      // (kernels.hip root_fold: the one store goes into the ROOT's recv, nothing into this rank's)
      if (W.coll == kCollReduce) {
        memcpy((char*)W.recv[W.root] + coff, res.data(), (size_t)len);
        return;
      }
      memcpy((char*)W.recv[r] + coff, res.data(), (size_t)len);
      // (kernels.hip scatter_fold: the fold with no pushes -- W.recv[r] is recv - r * chunk_bytes)
      if (W.coll == kCollReduceScatter) return;
      for (int k = 1; k < n; ++k) memcpy((char*)W.recv[direct_peer(n, r, k)] + coff, res.data(), (size_t)len);
    }
  };
  // kernels.hip gather_push: slice `it` of this rank's send (W.send[r] is send - r * chunk_bytes)
  // into chunk r of its own recv (not in place) and of every peer's
  auto push = [&](uint32_t it) {
    const uint64_t s = (uint64_t)it * W.A + w;
    const uint64_t len = slice_len(W.chunk_bytes, W.slice, s);
    const uint64_t coff = (uint64_t)r * W.chunk_bytes + s * W.slice;
    if (!len) return;
    const char* src = (const char*)W.send[r] + coff;
    if (W.own[(size_t)r]) memcpy((char*)W.recv[r] + coff, src, (size_t)len);
    for (int k = 1; k < n; ++k) memcpy((char*)W.recv[direct_peer(n, r, (k - 1 + w) % (n - 1) + 1)] + coff, src, (size_t)len);
  };
  // kernels.hip root_relay: slice `it` of chunk r of the ROOT's send into every rank's recv -- the
  // root's own only when its call is out of place (seen from the buffers, as the kernel does)
  auto relay = [&](uint32_t it) {
    const uint64_t s = (uint64_t)it * W.A + w;
    const uint64_t len = slice_bytes_of(s);
    const uint64_t coff = (uint64_t)r * W.chunk_bytes + s * W.slice;
    if (!len) return;
    const bool root_in_place = (const void*)W.send[W.root] == (const void*)W.recv[W.root];
    std::vector<char> v((const char*)W.send[W.root] + coff, (const char*)W.send[W.root] + coff + len);
    for (int q = 0; q < n; ++q)
      if (q != W.root || !root_in_place) memcpy((char*)W.recv[q] + coff, v.data(), (size_t)len);
  };
  // kernels.hip exchange_push: slice `it` of EVERY block q of this rank's send into block r of rank
  // q's recv, the peers in direct_peer order from peer w mod n-1, this rank's own block last
  auto exchange = [&](uint32_t it) {
    const uint64_t s = (uint64_t)it * W.A + w;
    const uint64_t len = slice_len(W.chunk_bytes, W.slice, s);
    const uint64_t soff = s * W.slice, mine = (uint64_t)r * W.chunk_bytes + soff;
    if (!len) return;
    for (int k = 0; k < n; ++k) {
      const int q = k < n - 1 ? direct_peer(n, r, 1 + (w % (n - 1) + k) % (n - 1)) : r;
      memcpy((char*)W.recv[q] + mine, (const char*)W.send[r] + (uint64_t)q * W.chunk_bytes + soff, (size_t)len);
    }
  };
  // kernels.hip collect_push: slice `it` of this rank's one block (W.send[r] is send - r * chunk_bytes)
  // into block r of the ROOT's recv; the root's own block unless its call is in place (seen from the
  // shifted pointers, as the kernel does); a non-root writes nothing of its own
  auto collect = [&](uint32_t it) {
    const uint64_t s = (uint64_t)it * W.A + w;
    const uint64_t len = slice_len(W.chunk_bytes, W.slice, s);
    const uint64_t coff = (uint64_t)r * W.chunk_bytes + s * W.slice;
    if (!len) return;
    if (r == W.root && (const void*)W.send[r] == (const void*)W.recv[r]) return;
    memcpy((char*)W.recv[W.root] + coff, (const char*)W.send[r] + coff, (size_t)len);
  };
  // kernels.hip deal_push, on the root only: slice `it` of EVERY block q of its send into rank q's
  // recv with no block offset on the destination side (W.peer_recv: the unshifted buffers), the
  // peers in direct_peer order from peer w mod n-1, its own block last (W.recv[r] is recv - r *
  // chunk_bytes) unless the call is in place
  auto deal = [&](uint32_t it) {
    const uint64_t s = (uint64_t)it * W.A + w;
    const uint64_t len = slice_len(W.chunk_bytes, W.slice, s), soff = s * W.slice;
    if (!len || r != W.root) return;
    const int K = n - 1 + ((const void*)W.send[r] != (const void*)W.recv[r] ? 1 : 0);
    for (int k = 0; k < K; ++k) {
      const int q = k < n - 1 ? direct_peer(n, r, 1 + (w % (n - 1) + k) % (n - 1)) : r;
      char* to = k < n - 1 ? (char*)W.peer_recv[(size_t)q] + soff : (char*)W.recv[r] + (uint64_t)r * W.chunk_bytes + soff;
      memcpy(to, (const char*)W.send[r] + (uint64_t)q * W.chunk_bytes + soff, (size_t)len);
    }
  };
  // kernels.hip varblock_push: slice `it` of the call's largest-block geometry; of the block for each
  // destination it covers schedule.h varblock_len bytes (0 once that block is exhausted)
  auto varexchange = [&](uint32_t it) {
    const uint64_t s = (uint64_t)it * W.A + w, soff = s * W.slice;
    for (int k = 0; k < n; ++k) {
      const int q = k < n - 1 ? direct_peer(n, r, 1 + (w % (n - 1) + k) % (n - 1)) : r;
      const size_t i = (size_t)r * n + q;
      const uint64_t len = varblock_len(W.vbytes[i], W.slice, s);
      if (len) memcpy((char*)W.recv[q] + W.vdst[i] + soff, (const char*)W.send[r] + W.vsrc[i] + soff, (size_t)len);
    }
  };
  // kernels.hip vhalf_fold: slice `it` of the largest-block geometry, clamped to this rank's own block
  // (schedule.h vhalf_len), folded out of every rank's send at hbase[r] in ring order into this rank's
  // recv (W.recv[r] is recv - hbase[r]); every load of the slice first (in place)
  auto vfold = [&](uint32_t it) {
    const uint64_t s = (uint64_t)it * W.A + w;
    const uint64_t len = vhalf_len(W.hbytes[r], W.slice, s), coff = W.hbase[r] + s * W.slice;
    if (!len) return;
    std::vector<float> res((size_t)(len / 4));
    for (uint64_t i = 0; i < len / 4; ++i) {
      float acc = ((const float*)((const char*)W.send[r] + coff))[i];
      for (int k = 1; k < n; ++k) acc = apply(W.op, ((const float*)((const char*)W.send[direct_peer(n, r, k)] + coff))[i], acc);
      res[(size_t)i] = acc;
    }
    memcpy((char*)W.recv[r] + coff, res.data(), (size_t)len);
  };
  // kernels.hip vhalf_push: the same slice of this rank's send (W.send[r] is send - hbase[r]) into
  // hbase[r] of its own recv (not in place) and of every peer's
  auto vpush = [&](uint32_t it) {
    const uint64_t s = (uint64_t)it * W.A + w;
    const uint64_t len = vhalf_len(W.hbytes[r], W.slice, s), coff = W.hbase[r] + s * W.slice;
    if (!len) return;
    const char* src = (const char*)W.send[r] + coff;
    if (W.own[(size_t)r]) memcpy((char*)W.recv[r] + coff, src, (size_t)len);
    for (int k = 1; k < n; ++k) memcpy((char*)W.recv[direct_peer(n, r, (k - 1 + w) % (n - 1) + 1)] + coff, src, (size_t)len);
  };
  switch (P.j) {
    case 0:
      // START (kernels.hip read_kernel).  A registered-window call's signature is stored with it but
      // not drained first, so it may land after the flag: modelled as a later step (stage 5)
      for (int k = 1; k < n; ++k) W.ready(direct_peer(n, r, k), r, w) = tx(direct_peer(n, r, k)) + 1;
      P.j = W.sig.empty() ? 1 : 5;
      return true;
    case 5:
      for (int k = 1; k < n; ++k) W.mbox[direct_peer(n, r, k)][mbox_ready(W.C, r, w) + kSigWord] = W.sig[r];
      P.j = 1;
      return true;
    case 1:
      for (int k = 1; k < n; ++k)
        if (W.ready(r, direct_peer(n, r, k), w) < rx(direct_peer(n, r, k)) + 1) return false;
      if (!W.sig.empty()) {  // kernels.hip starts_agree: wait for each signature, compare, clear
        for (int k = 1; k < n; ++k)
          if (W.mbox[r][mbox_ready(W.C, direct_peer(n, r, k), w) + kSigWord] == 0) return false;
        bool bad = false;
        for (int k = 1; k < n; ++k) {
          uint64_t& word = W.mbox[r][mbox_ready(W.C, direct_peer(n, r, k), w) + kSigWord];
          bad = bad || word != W.sig[r];
          word = 0;
        }
        if (bad) {
          ++W.mismatch[r];
          P.done = true;
          return true;
        }
      }
      P.j = 2;
      P.it = 0;
      P.k = 0;
      return true;
    case 2:
      if (P.it < W.iters) {
        if (W.coll == kCollAllGather) push(P.it++);
        else if (W.coll == kCollBroadcast) relay(P.it++);
        else if (W.coll == kCollAllToAll) exchange(P.it++);
        else if (W.coll == kCollAllToAllV) varexchange(P.it++);
        else if (W.coll == kCollAllGatherV) vpush(P.it++);
        else if (W.coll == kCollReduceScatterV) vfold(P.it++);
        else if (W.coll == kCollGather) collect(P.it++);
        else if (W.coll == kCollScatter) deal(P.it++);
        else fold(P.it++);
      }
      if (P.it >= W.iters) P.j = 3;
      return true;
    case 3:
      for (int k = 1; k < n; ++k) {
        const int q = direct_peer(n, r, k);
        W.credit(q, r, w) = rx(q) + mpc;
        W.ready(q, r, w) = tx(q) + mpc;
      }
      P.j = 4;
      return true;
    default:
      for (int k = 1; k < n; ++k)
        if (W.ready(r, direct_peer(n, r, k), w) < rx(direct_peer(n, r, k)) + mpc) return false;
      P.done = true;
      return true;
  }
}

// One step of the one-shot schedule (kernels.hip oneshot_kernel): pipeline w = s * n + c owns
// slice s of chunk c.  Stage 0 waits for every peer's credit, stores that piece of its send into
// every peer's slot and raises READY; stage 1 waits for every peer's READY, folds the piece in
// ring order from the slots (its own piece from its send) into recv and returns the credits.
bool oneshot_step(World& W, Prog& P) {
  const int n = W.n, r = P.r, w = P.w, K = W.K;
  auto tx = [&](int d) { return W.tx_seq[r][(size_t)d * W.C + w]; };
  auto rx = [&](int q) { return W.rx_seq[r][(size_t)q * W.C + w]; };
  const int c = w % n;
  const uint64_t s = (uint64_t)(w / n);
  const uint64_t len = slice_len(W.chunk_bytes, W.slice, s), coff = (uint64_t)c * W.chunk_bytes + s * W.slice;
  if (P.j == 0) {
    for (int k = 1; k < n; ++k) {
      const int q = direct_peer(n, r, k);
      if (tx(q) + 1 > (uint64_t)K && W.credit(r, q, w) < tx(q) + 1 - K) return false;
    }
    for (int k = 1; k < n; ++k) {
      const int q = direct_peer(n, r, k);
      if (len) memcpy(W.slot(r, q, w, tx(q)), (const char*)W.send[r] + coff, len);
      W.ready(q, r, w) = tx(q) + 1;
    }
    P.j = 1;
    return true;
  }
  for (int k = 1; k < n; ++k) {
    const int q = direct_peer(n, r, k);
    if (W.ready(r, q, w) < rx(q) + 1) return false;
  }
  auto piece = [&](int q) -> const float* {
    return (const float*)(q == r ? (const char*)W.send[r] + coff : W.slot(q, r, w, rx(q)));
  };
  if (len) {
    // every piece is read before recv's (in place: send's) piece is written
    std::vector<float> res((size_t)(len / 4));
    for (uint64_t i = 0; i < len / 4; ++i) {
      float acc = piece(c)[i];
      for (int k = 1; k < n; ++k) acc = apply(W.op, piece(direct_peer(n, c, k))[i], acc);
      res[(size_t)i] = acc;
    }
    memcpy((char*)W.recv[r] + coff, res.data(), (size_t)len);
  }
  for (int k = 1; k < n; ++k) {
    const int q = direct_peer(n, r, k);
    W.credit(q, r, w) = rx(q) + 1;
  }
  P.done = true;
  return true;
}

// a fresh communicator state: scratch, mailboxes and the per-pair FIFO counters, all zero
void init_world(World& W, int n, int channels, int slots, int op, uint64_t slice_bytes) {
  W.n = n; W.C = channels; W.K = slots; W.op = op; W.algo = 0; W.slot_bytes = slice_bytes;
  // n - 1 regions per rank, exactly as Comm allocates (schedule.h region_index)
  W.scratch.assign((size_t)n, std::vector<char>((size_t)(n > 1 ? n - 1 : 1) * scratch_region_bytes(channels, slots, slice_bytes)));
  W.mbox.assign((size_t)n, std::vector<uint64_t>((size_t)mbox_words(n, channels), 0));
  W.tx_seq.assign((size_t)n, std::vector<uint64_t>((size_t)n * channels, 0));
  W.rx_seq.assign((size_t)n, std::vector<uint64_t>((size_t)n * channels, 0));
}

// One call on the state W, as Comm::collective + Comm::launch run it: schedule `code` (0 ring,
// 1 one-shot, 2 read (persistent kernel), 4 read's grid form), collective `coll` over `count`
// elements (the all-reduce's; per rank for a half).  0, -1 on deadlock, -2 on bad arguments.
int run_call(World& W, int code, int coll, uint64_t count, const float* const* send, float* const* recv,
             uint64_t slice_bytes, uint64_t min_slice, uint64_t schedule_seed, uint64_t& rng, uint64_t& steps,
             int root = 0) {
  const int n = W.n, channels = W.C;
  const bool rooted = coll == kCollBroadcast || coll == kCollReduce;
  const bool gs = coll == kCollGather || coll == kCollScatter;
  const bool half = coll != kCollAllReduce;  // (the rooted ones too: ring and persistent read only)
  if (code > 4 || code == 3 || (half && code != 0 && code != 2)) return -2;
  if ((rooted || gs) && (root < 0 || root >= n)) return -2;
  const int a = code >= 2 ? 2 : code;  // 0 ring, 1 one-shot, 2 read
  const uint64_t chunk = rooted ? (count + (uint64_t)n - 1) / (uint64_t)n : half ? count : count / (uint64_t)n;
  W.coll = coll;
  W.root = root;
  W.total_bytes = rooted ? count * 4 : 0;
  W.chunk_bytes = chunk * 4;
  if (coll == kCollAllToAllV) W.chunk_bytes = count;  // (run_var_call: the largest block, in bytes)
  const bool vhalf = coll == kCollAllGatherV || coll == kCollReduceScatterV;
  if (vhalf) W.chunk_bytes = count;  // (run_vhalf_call: the largest block, in bytes)
  W.send.assign(send, send + n);
  W.recv.assign(recv, recv + n);
  if (!vhalf) W.own.assign((size_t)n, 1);  // (run_vhalf_call has set it and shifted the pointers)
  if (gs) {
    // Comm::collective: a non-root's large buffer (it may be NULL) is stood in for by its one-block
    // buffer; one rank: a copy; on the ring the root's own block reaches its place by a copy before
    // the launch when the call is not in place; then the one-block buffer's pointer shifted by r
    // blocks (Comm::make_params) -- the peers' mappings of a recv stay unshifted
    for (int r = 0; r < n; ++r) {
      if (r == root) continue;
      if (coll == kCollGather) W.recv[r] = const_cast<float*>(W.send[r]);
      else W.send[r] = W.recv[r];
    }
    if (n == 1) {
      if ((const void*)send[0] != (const void*)recv[0]) memcpy(recv[0], send[0], (size_t)W.chunk_bytes);
      return 0;
    }
    W.peer_recv = W.recv;
    const uint64_t mine = (uint64_t)root * W.chunk_bytes;
    const char* s = (const char*)send[root];
    char* d = (char*)recv[root];
    if (a == 0 && coll == kCollGather && s != d + mine) memcpy(d + mine, s, (size_t)W.chunk_bytes);
    if (a == 0 && coll == kCollScatter && d != s + mine) memcpy(d, s + mine, (size_t)W.chunk_bytes);
    for (int r = 0; r < n; ++r) {
      if (coll == kCollGather) W.send[r] = (const float*)((const char*)W.send[r] - (uint64_t)r * W.chunk_bytes);
      else W.recv[r] = (float*)((char*)W.recv[r] - (uint64_t)r * W.chunk_bytes);
    }
  }
  if (rooted) {
    // Comm::collective: the buffer a rank's role does not use (it may be NULL) is stood in for by
    // its other buffer; one rank: a copy; the ring's broadcast moves the whole buffer as one chunk
    // and the root's recv, out of place, gets its send by a copy before the launch
    for (int r = 0; r < n; ++r) {
      if (r == root) continue;
      if (coll == kCollBroadcast) W.send[r] = W.recv[r];
      else W.recv[r] = const_cast<float*>(W.send[r]);
    }
    if (n == 1) {
      if ((const void*)send[0] != (const void*)recv[0]) memcpy(recv[0], send[0], count * 4);
      return 0;
    }
    if (coll == kCollBroadcast && a == 0) {
      W.chunk_bytes = W.total_bytes;
      if ((const void*)send[root] != (const void*)recv[root]) memcpy(recv[root], send[root], count * 4);
    }
  }
  // as Comm::launch: adaptive payload (min_slice 0 = off; the read schedule's own rule), fixed
  // slot stride, one pipeline per slice up to all of them
  if (a == 1 && W.chunk_bytes) {
    if (min_slice && !oneshot_fits(W.chunk_bytes, n, channels, slice_bytes, true)) return -2;
    W.slice = min_slice ? oneshot_slice(W.chunk_bytes, n, channels, slice_bytes) : slice_bytes;
    if ((W.chunk_bytes + W.slice - 1) / W.slice * (uint64_t)n > (uint64_t)channels) return -2;
  } else if (!min_slice || a == 1) W.slice = slice_bytes;
  else if (a == 2) W.slice = read_slice(W.chunk_bytes, channels, slice_bytes, min_slice, kReadDepth);
  else W.slice = effective_slice(W.chunk_bytes, channels, slice_bytes, min_slice, 1);
  if (code == 4 && W.chunk_bytes) W.slice = W.chunk_bytes;  // grid form: one "slice", pipeline 0's protocol
  W.nslices = (W.chunk_bytes + W.slice - 1) / W.slice;
  W.A = call_pipelines(a == 1 ? W.nslices * (uint64_t)n : W.nslices, channels, 1);  // one-shot: per chunk too
  W.iters = (uint32_t)((W.nslices + (uint64_t)W.A - 1) / (uint64_t)W.A);
  for (int r = 0; r < n && !rooted && !gs; ++r) {
    if (half) {
      // Comm::collective: one device copy of the chunk with one rank; the ring's all-gather gets
      // the own chunk by a copy before the launch when the call is not in place; then the
      // one-chunk buffer's pointer shifted by r chunks (Comm::launch)
      const char* s = (const char*)send[r];
      char* d = (char*)recv[r];
      if (n == 1) {
        if (s != d) memcpy(d, s, (size_t)W.chunk_bytes);
        continue;
      }
      if (coll == kCollAllToAllV || vhalf) continue;  // read schedule only: the kernel moves the own block too
      if (coll == kCollAllToAll) {
        // no pointer shift and no in-place form; the ring moves the blocks between ranks only, the
        // own block reaches the own recv by a copy before the launch (Comm::collective)
        if (a == 0) memcpy(d + (uint64_t)r * W.chunk_bytes, s + (uint64_t)r * W.chunk_bytes, (size_t)W.chunk_bytes);
      } else if (coll == kCollAllGather) {
        W.own[(size_t)r] = s != d + (uint64_t)r * W.chunk_bytes;
        if (a == 0 && W.own[(size_t)r]) memcpy(d + (uint64_t)r * W.chunk_bytes, s, (size_t)W.chunk_bytes);
        W.send[r] = (const float*)(s - (uint64_t)r * W.chunk_bytes);
      } else {
        W.recv[r] = (float*)(d - (uint64_t)r * W.chunk_bytes);
      }
      continue;
    }
    // send -> recv copy of the tail (Comm::collective)
    if ((const void*)recv[r] == (const void*)send[r]) continue;  // in place
    const uint64_t body = W.chunk_bytes * (uint64_t)n;
    if (n == 1 || chunk == 0) memcpy(recv[r], send[r], count * 4);
    else if (count * 4 > body) memcpy((char*)recv[r] + body, (const char*)send[r] + body, count * 4 - body);
  }
  if (n == 1 || chunk == 0) return 0;
  std::vector<Prog> progs;
  for (int r = 0; r < n; ++r)
    for (int w = 0; w < channels; ++w) {
      Prog p;
      p.r = r; p.w = w;
      p.done = W.iters == 0 || w >= W.A;  // pipelines past A sit the call out
      progs.push_back(p);
    }
  for (;;) {
    bool any = false, all_done = true;
    const size_t np = progs.size();
    const size_t start = schedule_seed ? (size_t)((rng >> 33) % np) : 0;
    for (size_t j = 0; j < np; ++j) {
      Prog& P = progs[(start + j) % np];
      if (P.done) continue;
      all_done = false;
      // a random number of ops per turn for this program when seeded
      int burst = 1;
      if (schedule_seed) {
        rng = rng * 6364136223846793005ull + 1442695040888963407ull;
        burst = 1 + (int)((rng >> 40) % 4);
      }
      for (int b = 0; b < burst && !P.done; ++b) {
        const bool ok = a == 2 ? read_step(W, P) : a == 1 ? oneshot_step(W, P) : ring_step(W, P);
        if (!ok) break;
        any = true;
        ++steps;
      }
    }
    if (schedule_seed) rng = rng * 6364136223846793005ull + 1442695040888963407ull;
    if (all_done) break;
    if (!any) return -1;  // deadlock
  }
  // the kernels' last action per pipeline that ran: advance the per-pair FIFO counters
  for (int r = 0; r < n; ++r)
    for (int w = 0; w < W.A; ++w) {
      if (a == 2 || a == 1) {
        const uint64_t m = a == 2 ? read_msgs_per_call(W.iters) : 1;  // one-shot: one message each way
        for (int q = 0; q < n; ++q) {
          if (q == r) continue;
          W.tx_seq[r][(size_t)q * channels + w] += m;
          W.rx_seq[r][(size_t)q * channels + w] += m;
        }
      } else {
        W.tx_seq[r][(size_t)mod_n(r + 1, n) * channels + w] += (uint64_t)W.iters * coll_tx_msgs(coll, n, r, root);
        W.rx_seq[r][(size_t)mod_n(r - 1, n) * channels + w] += (uint64_t)W.iters * coll_rx_msgs(coll, n, r, root);
      }
    }
  return 0;
}

// One ncclAllToAllv call on the state W, as Comm::all_to_all_v runs it.  counts / sdispls / rdispls:
// n x n, in elements of esz bytes -- [r * n + q] is rank r's entry for peer q.  The caller has checked
// the matrix (varblock.h).  The geometry follows M, the largest block in bytes.  Read (code 2):
// kernels.hip varblock_push through read_step.  Ring (code 0): the blocks packed at q * Mpad of a
// stage, the ring's all-to-all with chunk Mpad into a second stage, unpacked into recv at rdispls;
// the own block one direct copy.
int run_var_call(World& W, int code, int esz, const uint64_t* counts, const uint64_t* sdispls, const uint64_t* rdispls,
                 const char* const* send, char* const* recv, uint64_t slice_bytes, uint64_t min_slice,
                 uint64_t schedule_seed, uint64_t& rng, uint64_t& steps) {
  const int n = W.n;
  if (code != 0 && code != 2) return -2;
  uint64_t M = 0;
  for (int i = 0; i < n * n; ++i) M = counts[i] * (uint64_t)esz > M ? counts[i] * (uint64_t)esz : M;
  if (n == 1) {
    if (M) memcpy(recv[0] + rdispls[0] * esz, send[0] + sdispls[0] * esz, (size_t)M);
    return 0;
  }
  if (M == 0) return 0;  // nothing launched
  if (code == 2) {
    std::vector<uint64_t> vb((size_t)n * n), vs((size_t)n * n), vd((size_t)n * n);
    for (int r = 0; r < n; ++r)
      for (int q = 0; q < n; ++q) {
        vb[(size_t)r * n + q] = counts[(size_t)r * n + q] * (uint64_t)esz;
        vs[(size_t)r * n + q] = sdispls[(size_t)r * n + q] * (uint64_t)esz;
        vd[(size_t)r * n + q] = rdispls[(size_t)q * n + r] * (uint64_t)esz;  // rank q's displacement for source r
      }
    W.vbytes = vb.data();
    W.vsrc = vs.data();
    W.vdst = vd.data();
    const int rc = run_call(W, 2, kCollAllToAllV, M, (const float* const*)send, (float* const*)recv, slice_bytes, min_slice,
                            schedule_seed, rng, steps);
    W.vbytes = W.vsrc = W.vdst = nullptr;
    return rc;
  }
  const uint64_t Mpad = (M + 15) & ~(uint64_t)15;
  std::vector<std::vector<char>> in((size_t)n, std::vector<char>((size_t)(n * Mpad), (char)0x5c)),
      out((size_t)n, std::vector<char>((size_t)(n * Mpad), (char)0x5c));
  std::vector<const float*> sp((size_t)n);
  std::vector<float*> rp((size_t)n);
  for (int r = 0; r < n; ++r) {
    for (int q = 0; q < n; ++q)
      if (q != r && counts[(size_t)r * n + q])
        memcpy(in[(size_t)r].data() + (size_t)q * Mpad, send[r] + sdispls[(size_t)r * n + q] * esz,
               (size_t)(counts[(size_t)r * n + q] * esz));
    sp[(size_t)r] = (const float*)in[(size_t)r].data();
    rp[(size_t)r] = (float*)out[(size_t)r].data();
  }
  const int rc = run_call(W, 0, kCollAllToAll, Mpad / 4, sp.data(), rp.data(), slice_bytes, min_slice, schedule_seed, rng,
                          steps);
  if (rc != 0) return rc;
  for (int r = 0; r < n; ++r)
    for (int q = 0; q < n; ++q) {
      const uint64_t c = counts[(size_t)q * n + r] * (uint64_t)esz;  // what q sent to r
      if (!c) continue;
      const char* from = q == r ? send[r] + sdispls[(size_t)r * n + r] * esz : out[(size_t)r].data() + (size_t)q * Mpad;
      memcpy(recv[r] + rdispls[(size_t)r * n + q] * esz, from, (size_t)c);
    }
  return 0;
}

// One mncclAllGatherv (coll 9) / mncclReduceScatterv (coll 10) call on the state W, as Comm::vhalf runs
// it.  counts / displs: n entries in elements of esz bytes, the same on every rank (the caller has
// checked the rules, vhalves.h); array[r] rank r's buffer with the n blocks (the gather's recv, the
// scatter's send), one[r] its one block (NULL allowed where counts[r] is 0).  The geometry follows M,
// the largest block in bytes.  Read (code 2): kernels.hip vhalf_push / vhalf_fold through read_step,
// the one-block buffer's pointer shifted by -base.  Ring (code 0): an n * Mpad stage per rank in the
// in-place layout -- the gather packs its block into chunk r, runs the ring all-gather and unpacks the
// n blocks; the scatter packs the n blocks, runs the ring reduce-scatter and copies chunk r out.
// The fold is fp32 (esz 4), as everywhere in this simulator.
int run_vhalf_call(World& W, int code, int coll, int esz, const uint64_t* counts, const uint64_t* displs,
                   char* const* array, char* const* one, uint64_t slice_bytes, uint64_t min_slice, uint64_t schedule_seed,
                   uint64_t& rng, uint64_t& steps) {
  const int n = W.n;
  const bool gather = coll == kCollAllGatherV;
  if ((code != 0 && code != 2) || (!gather && esz != 4)) return -2;
  uint64_t M = 0;
  for (int q = 0; q < n; ++q) M = counts[q] * (uint64_t)esz > M ? counts[q] * (uint64_t)esz : M;
  if (M == 0) return 0;  // nothing launched
  if (n == 1) {
    char* blk = array[0] + displs[0] * esz;
    if (blk != one[0]) memcpy(gather ? blk : one[0], gather ? one[0] : blk, (size_t)M);
    return 0;
  }
  if (code == 2) {
    std::vector<uint64_t> hb((size_t)n), hl((size_t)n);
    std::vector<const float*> sp((size_t)n);
    std::vector<float*> rp((size_t)n);
    W.own.assign((size_t)n, 1);
    for (int r = 0; r < n; ++r) {
      hl[(size_t)r] = counts[r] * (uint64_t)esz;
      hb[(size_t)r] = counts[r] ? displs[r] * (uint64_t)esz : 0;  // an empty block's displacement is never used
      // Comm::vhalf: a NULL one-block buffer is stood in for by the other; then shifted by -base
      char* o = one[r] ? one[r] : array[r];
      sp[(size_t)r] = (const float*)(gather ? o - hb[(size_t)r] : array[r]);
      rp[(size_t)r] = (float*)(gather ? array[r] : o - hb[(size_t)r]);
      W.own[(size_t)r] = (const void*)sp[(size_t)r] != (const void*)rp[(size_t)r];
    }
    W.hbase = hb.data();
    W.hbytes = hl.data();
    const int rc = run_call(W, 2, coll, M, sp.data(), rp.data(), slice_bytes, min_slice, schedule_seed, rng, steps);
    W.hbase = W.hbytes = nullptr;
    return rc;
  }
  const uint64_t Mpad = (M + 15) & ~(uint64_t)15;
  std::vector<std::vector<char>> stage((size_t)n, std::vector<char>((size_t)(n * Mpad), (char)0x5c));
  std::vector<const float*> sp((size_t)n);
  std::vector<float*> rp((size_t)n);
  for (int r = 0; r < n; ++r) {
    char* st = stage[(size_t)r].data();
    if (gather) {
      if (counts[r]) memcpy(st + (size_t)r * Mpad, one[r], (size_t)(counts[r] * esz));
    } else {
      for (int q = 0; q < n; ++q)
        if (counts[q]) memcpy(st + (size_t)q * Mpad, array[r] + displs[q] * esz, (size_t)(counts[q] * esz));
    }
    sp[(size_t)r] = (const float*)(gather ? st + (size_t)r * Mpad : st);
    rp[(size_t)r] = (float*)(gather ? st : st + (size_t)r * Mpad);
  }
  const int rc = run_call(W, 0, gather ? kCollAllGather : kCollReduceScatter, Mpad / 4, sp.data(), rp.data(), slice_bytes,
                          min_slice, schedule_seed, rng, steps);
  if (rc != 0) return rc;
  for (int r = 0; r < n; ++r) {
    const char* st = stage[(size_t)r].data();
    if (!gather) {
      if (counts[r]) memcpy(one[r], st + (size_t)r * Mpad, (size_t)(counts[r] * esz));
      continue;
    }
    for (int q = 0; q < n; ++q) {
      char* blk = array[r] + displs[q] * esz;
      if (!counts[q] || (q == r && one[r] == blk)) continue;  // (in place: the own block is there)
      memcpy(blk, q == r ? one[r] : st + (size_t)q * Mpad, (size_t)(counts[q] * esz));
    }
  }
  return 0;
}

// ---- point to point (kernels.hip p2p_kernel, and p2p_window_group on registered windows) ----
// One wave of a launch: pair `pair` of the launch's argument on pipeline w, at operation i, slice s.
struct P2pWave {
  int pair, w, i;
  uint64_t s, seq;
  bool done = false;
  // the window kernel: whether the current message's hand-off happened, and what it said
  bool handed = false, direct = false;
  char* dest = nullptr;
};

// the simulated windows: window k is win_base[k * n + q] on rank q, win_bytes[k] bytes; its table slot is k
struct SimWindows {
  int nwin = 0;
  void* const* base = nullptr;
  const uint64_t* bytes = nullptr;
};

struct P2pLaunch {
  P2pWinArgs wa;     // (wa.a alone for p2p_kernel)
  bool win = false;  // the window kernel's protocol: a DEST record per message
  std::vector<P2pWave> waves;
};

// the launch's waves as the kernel maps them (wave b: pair b / pipes, pipeline b % pipes); the self
// copies happen at once (their waves wait for nobody)
void p2p_start(World& W, int r, P2pLaunch& L) {
  const P2pArgs& a = L.wa.a;
  for (int c = 0; c < a.nself; ++c) {
    const int i = a.self_first + 2 * c;
    memcpy((void*)(uintptr_t)a.ptr[i + 1], (const void*)(uintptr_t)a.ptr[i], (size_t)a.bytes[i]);
  }
  L.waves.clear();
  for (int b = 0; b < a.npairs * a.pipes; ++b) {
    P2pWave v;
    v.pair = b / a.pipes;
    v.w = b % a.pipes;
    v.i = a.pair_first[v.pair];
    v.s = (uint64_t)v.w;
    const int peer = a.pair_peer[v.pair];
    v.seq = (a.pair_send[v.pair] ? W.tx_seq : W.rx_seq)[r][(size_t)peer * W.C + v.w];
    L.waves.push_back(v);
  }
}

// One step of one wave -- a slice, a direct message's hand-off and push, or its end (the counter
// written back): 1, 0 if its wait is unsatisfied, -4 when a sender refuses the receiver's record.
// direct[0] / direct[1]: rank r's recvs posted direct / messages pushed direct.
int p2p_step(World& W, int r, const P2pLaunch& L, P2pWave& v, const SimWindows& T, uint64_t* direct) {
  const P2pArgs& a = L.wa.a;
  const int peer = a.pair_peer[v.pair], w = v.w, K = W.K, n = W.n;
  const bool sends = a.pair_send[v.pair] != 0;
  const int last = a.pair_first[v.pair] + a.pair_count[v.pair];
  for (;;) {
    if (v.i >= last) {
      (sends ? W.tx_seq : W.rx_seq)[r][(size_t)peer * W.C + w] = v.seq;
      v.done = true;
      return 1;
    }
    const uint64_t bytes = a.bytes[v.i], nsl = p2p_nslices(bytes, W.slot_bytes);
    const int A = p2p_msg_pipes(bytes, W.slot_bytes, a.p2p_pipes);
    if (w >= A || v.s >= nsl) {  // the next operation of the pair
      ++v.i;
      v.s = (uint64_t)w;
      v.handed = false;
      continue;
    }
    const uint64_t mine = p2p_pipe_msgs(bytes, W.slot_bytes, a.p2p_pipes, w);
    if (L.win && !v.handed) {  // kernels.hip p2p_window_group: the message's DEST record
      if (!sends) {
        P2pDest d;
        d.tag = p2p_dest_tag(v.seq);
        d.direct = L.wa.wslot[v.i] != kP2pNoSlot ? 1u : 0u;
        d.slot = d.direct ? L.wa.wslot[v.i] : 0u;
        d.off = d.direct ? L.wa.woff[v.i] : 0;
        d.bytes = bytes;
        uint64_t* info = &W.mbox[peer][mbox_dest_info(n, W.C, r, w)];
        p2p_dest_encode(d, info);
        W.mbox[peer][mbox_dest_tag(n, W.C, r, w)] = d.tag;
        v.direct = d.direct != 0;
        if (v.direct && w == 0) ++direct[0];
      } else {
        const uint64_t tag = W.mbox[r][mbox_dest_tag(n, W.C, peer, w)];
        if (tag < p2p_dest_tag(v.seq)) return 0;
        const P2pDest d = p2p_dest_decode(&W.mbox[r][mbox_dest_info(n, W.C, peer, w)], tag);
        const bool slot_ok = d.direct && d.slot < (uint32_t)T.nwin;
        const uint64_t wbase = slot_ok ? (uint64_t)(uintptr_t)T.base[(size_t)d.slot * n + peer] : 0;
        const uint64_t wbytes = slot_ok ? T.bytes[d.slot] : 0;
        if (d.tag != p2p_dest_tag(v.seq) || p2p_dest_check(d, bytes, wbase, wbytes) != kDestOk) return -4;
        v.direct = d.direct != 0;
        v.dest = (char*)(uintptr_t)(wbase + d.off);
      }
      v.handed = true;
      if (!sends) return 1;  // (posting is a step of its own: the sender may run in between)
    }
    if (L.win && v.direct) {
      if (sends) {  // slices w, w + A, ... straight into the peer's recv; READY once
        for (uint64_t s = (uint64_t)w; s < nsl; s += (uint64_t)A)
          memcpy(v.dest + s * W.slot_bytes, (const char*)(uintptr_t)a.ptr[v.i] + s * W.slot_bytes,
                 (size_t)slice_len(bytes, W.slot_bytes, s));
        W.ready(peer, r, w) = v.seq += mine;
        if (w == 0) ++direct[1];
      } else {
        if (W.ready(r, peer, w) < v.seq + mine) return 0;
        W.credit(peer, r, w) = v.seq += mine;
      }
      v.s = nsl;
      return 1;
    }
    const uint64_t len = slice_len(bytes, W.slot_bytes, v.s);
    char* at = (char*)(uintptr_t)a.ptr[v.i] + v.s * W.slot_bytes;
    if (sends) {
      if (v.seq + 1 > (uint64_t)K && W.credit(r, peer, w) < v.seq + 1 - K) return 0;
      memcpy(W.slot(r, peer, w, v.seq), at, (size_t)len);
      W.ready(peer, r, w) = ++v.seq;
    } else {
      if (W.ready(r, peer, w) < v.seq + 1) return 0;
      memcpy(at, W.slot(peer, r, w, v.seq), (size_t)len);
      W.credit(peer, r, w) = ++v.seq;
    }
    v.s += (uint64_t)A;
    return 1;
  }
}

// One point-to-point phase: rank r runs launches[r] one after another (stream order), the ranks
// independently of each other.  0, -1 on no progress.
int run_p2p_phase(World& W, std::vector<std::vector<P2pLaunch>>& launches, uint64_t schedule_seed, uint64_t& rng,
                  uint64_t& steps, const SimWindows& T, uint64_t* direct) {
  const int n = W.n;
  std::vector<size_t> cur((size_t)n, 0);
  for (int r = 0; r < n; ++r)
    if (!launches[(size_t)r].empty()) p2p_start(W, r, launches[(size_t)r][0]);
  for (;;) {
    bool any = false, all_done = true;
    const int r0 = schedule_seed ? (int)((rng >> 33) % (uint64_t)n) : 0;
    for (int k = 0; k < n; ++k) {
      const int r = (r0 + k) % n;
      if (cur[(size_t)r] >= launches[(size_t)r].size()) continue;
      all_done = false;
      P2pLaunch& L = launches[(size_t)r][cur[(size_t)r]];
      bool launch_done = true;
      const size_t nw = L.waves.size();
      const size_t w0 = schedule_seed && nw ? (size_t)((rng >> 20) % nw) : 0;
      for (size_t j = 0; j < nw; ++j) {
        P2pWave& v = L.waves[(w0 + j) % nw];
        if (v.done) continue;
        int burst = 1;
        if (schedule_seed) {
          rng = rng * 6364136223846793005ull + 1442695040888963407ull;
          burst = 1 + (int)((rng >> 40) % 4);
        }
        for (int b = 0; b < burst && !v.done; ++b) {
          const int rc = p2p_step(W, r, L, v, T, direct + 2 * r);
          if (rc < 0) return rc;
          if (!rc) break;
          any = true;
          ++steps;
        }
        launch_done = launch_done && v.done;
      }
      if (launch_done) {  // the kernel ended: the rank's next launch starts
        any = true;
        if (++cur[(size_t)r] < launches[(size_t)r].size()) p2p_start(W, r, launches[(size_t)r][cur[(size_t)r]]);
      }
    }
    if (schedule_seed) rng = rng * 6364136223846793005ull + 1442695040888963407ull;
    if (all_done) return 0;
    if (!any) return -1;
  }
}

// The run behind mnccl_sim_p2p and mnccl_sim_p2p_win (below).  op_window == nullptr: p2p_kernel's
// protocol; else the window kernel's, operation k's recv posted direct into window op_window[k] (its
// table slot) or, with -1, through the scratch.
int sim_p2p_run(int n, int channels, int slots, uint64_t slot_bytes, int pipes, int nphases, const int* phase_coll,
                const int* phase_sched, const uint64_t* phase_count, const float* const* csend, float* const* crecv,
                int op, int nops, const int* op_phase, const int* op_rank, const int* op_launch, const int* op_send,
                const int* op_peer, void* const* op_ptr, const uint64_t* op_bytes, const int* op_window,
                const SimWindows& T, uint64_t schedule_seed, uint64_t* counters_out, uint64_t* direct_out,
                uint64_t* steps_out) {
  if (n < 1 || n > 16 || channels < 1 || slots < 1 || slot_bytes < 4 || slot_bytes % 4 || nphases < 0 || nops < 0 ||
      pipes < 1 || pipes > channels)
    return -2;
  if (op_window && (T.nwin < 0 || T.nwin > kP2pWinSlots)) return -2;
  World W;
  init_world(W, n, channels, slots, op, slot_bytes);
  std::vector<uint64_t> direct((size_t)2 * n, 0);
  uint64_t steps = 0;
  uint64_t rng = schedule_seed * 6364136223846793005ull + 1442695040888963407ull;
  int k = 0;
  for (int ph = 0; ph < nphases; ++ph) {
    if (phase_coll[ph] >= 0) {
      const int c = phase_coll[ph];
      if (c > kCollAllToAll || phase_count[ph] == 0) return -2;
      const int rc = run_call(W, phase_sched[ph], c, phase_count[ph], csend + (size_t)ph * n, crecv + (size_t)ph * n,
                              slot_bytes, 0, schedule_seed, rng, steps);
      if (rc != 0) return rc;
      continue;
    }
    std::vector<std::vector<P2pLaunch>> launches((size_t)n);
    while (k < nops && op_phase[k] == ph) {
      const int r = op_rank[k], l = op_launch[k];
      if (r < 0 || r >= n) return -2;
      P2pGroup g;
      uint8_t g_slot[kMaxGroupOps];
      uint64_t g_off[kMaxGroupOps];
      for (; k < nops && op_phase[k] == ph && op_rank[k] == r && op_launch[k] == l; ++k) {
        if (op_bytes[k] == 0) continue;  // count == 0: nothing recorded
        uint64_t bytes = 0;
        if (p2p_check_op(g, n, op_send[k] != 0, op_peer[k], op_ptr[k], (size_t)op_bytes[k], 1, &bytes) != kP2pOk) return -3;
        if (p2p_append(g, op_send[k] != 0, op_peer[k], op_ptr[k], (uint64_t)(uintptr_t)op_ptr[k], bytes) != kP2pOk) return -3;
        // Comm::p2p_group's decision per recv: the range lies in the window the caller names
        const int j = g.nops - 1, win = op_window ? op_window[k] : -1;
        g_slot[j] = (uint8_t)kP2pNoSlot;
        g_off[j] = 0;
        if (win < 0 || op_send[k] != 0 || op_peer[k] == r) continue;
        if (win >= T.nwin) return -2;
        const char* base = (const char*)T.base[(size_t)win * n + r];
        const char* at = (const char*)op_ptr[k];
        if (at < base || (uint64_t)(at - base) > T.bytes[win] || bytes > T.bytes[win] - (uint64_t)(at - base)) return -2;
        if (!p2p_win_direct(true, win, true)) continue;
        g_slot[j] = (uint8_t)win;
        g_off[j] = (uint64_t)(at - base);
      }
      P2pLaunch L;
      L.win = op_window != nullptr;
      if (p2p_win_build(g, r, pipes, slot_bytes, g_slot, g_off, &L.wa) != kP2pOk) return -3;
      if (p2p_launch_waves(L.wa.a) > 0) launches[(size_t)r].push_back(L);
    }
    const int rc = run_p2p_phase(W, launches, schedule_seed, rng, steps, T, direct.data());
    if (rc != 0) return rc;
  }
  if (k != nops) return -2;
  if (counters_out) {
    const size_t per = (size_t)n * channels;
    for (int r = 0; r < n; ++r)
      for (size_t j = 0; j < per; ++j) {
        counters_out[(size_t)r * per + j] = W.tx_seq[r][j];
        counters_out[(size_t)n * per + (size_t)r * per + j] = W.rx_seq[r][j];
      }
  }
  if (direct_out) memcpy(direct_out, direct.data(), direct.size() * sizeof(uint64_t));
  if (steps_out) *steps_out = steps;
  return 0;
}

}  // namespace

extern "C" {

// csrc/schedule.h point-to-point geometry, exported for the host-logic tests
int mnccl_resident_cap(int waves, int cus, int most, int waves_per_simd) { return resident_cap(waves, cus, most, waves_per_simd); }
int mnccl_p2p_pipes(int n, int channels, int cus, int most, int waves_per_simd) {
  return p2p_pipes(n, channels, cus, most, waves_per_simd);
}
int mnccl_p2p_msg_pipes(uint64_t bytes, uint64_t slot_bytes, int pipes) { return p2p_msg_pipes(bytes, slot_bytes, pipes); }
uint64_t mnccl_p2p_pipe_msgs(uint64_t bytes, uint64_t slot_bytes, int pipes, int w) {
  return p2p_pipe_msgs(bytes, slot_bytes, pipes, w);
}
int mnccl_p2p_max_group_ops(void) { return kMaxGroupOps; }

// Point-to-point groups between collectives on one simulated communicator state.  The run is a list
// of phases: phase_coll[i] >= 0 is one collective call (schedule.h Coll 0..5 on schedule
// phase_sched[i] over phase_count[i] elements, rank r's buffers csend / crecv[i * n + r], as
// mnccl_sim_mixed; root 0), phase_coll[i] == -1 a point-to-point phase.  The operations of all
// point-to-point phases are listed flat, sorted by (phase, rank, launch): operation k belongs to
// launch op_launch[k] of rank op_rank[k] in phase op_phase[k] -- a launch is one group, or one
// ungrouped call -- and is a send (op_send[k] != 0) or recv of op_bytes[k] bytes at op_ptr[k] with
// peer op_peer[k].  Within a phase every rank runs its launches in order, independently of the other
// ranks, each launch with kernels.hip p2p_kernel's wave-per-(pair, pipeline) mapping (p2p.h
// p2p_build with `pipes` = schedule.h p2p_pipes) on the real slot / flag / counter layout.
// counters_out (2 * n * n * channels words): every rank's tx then rx counters, [r][peer * channels + w].
// Returns 0, -1 on no progress, -2 on bad arguments, -3 when a group fails p2p.h's checks.
int mnccl_sim_p2p(int n, int channels, int slots, uint64_t slot_bytes, int pipes, int nphases, const int* phase_coll,
                  const int* phase_sched, const uint64_t* phase_count, const float* const* csend, float* const* crecv,
                  int op, int nops, const int* op_phase, const int* op_rank, const int* op_launch, const int* op_send,
                  const int* op_peer, void* const* op_ptr, const uint64_t* op_bytes, uint64_t schedule_seed,
                  uint64_t* counters_out, uint64_t* steps_out) {
  return sim_p2p_run(n, channels, slots, slot_bytes, pipes, nphases, phase_coll, phase_sched, phase_count, csend, crecv, op,
                     nops, op_phase, op_rank, op_launch, op_send, op_peer, op_ptr, op_bytes, nullptr, SimWindows(),
                     schedule_seed, counters_out, nullptr, steps_out);
}

// The same run on a communicator with registered windows (kernels.hip p2p_window_group): every
// launch runs the window kernel's protocol on the real word layout -- per message a DEST record in
// the sender's mailbox (schedule.h mbox_dest_info / mbox_dest_tag, p2p.h P2pDest), checked by the
// sender (p2p_dest_check) before it moves anything.  There are nwin <= kP2pWinSlots windows, window k
// being win_base[k * n + q] on rank q and win_bytes[k] bytes, in table slot k.  op_window[k] is the
// per-operation "in window" flag: -1 posts a recv "scratch" (and is what every send carries), a
// window's index posts it "direct" into that window, in which its range must lie (-2 if not).
// direct_out (2 * n words): per rank, the recvs it posted direct and the messages it pushed direct.
// Returns what mnccl_sim_p2p returns, and -4 when a sender refuses a record (the byte counts of a
// send and its recv differ).
int mnccl_sim_p2p_win(int n, int channels, int slots, uint64_t slot_bytes, int pipes, int nphases, const int* phase_coll,
                      const int* phase_sched, const uint64_t* phase_count, const float* const* csend,
                      float* const* crecv, int op, int nops, const int* op_phase, const int* op_rank,
                      const int* op_launch, const int* op_send, const int* op_peer, void* const* op_ptr,
                      const uint64_t* op_bytes, const int* op_window, int nwin, void* const* win_base,
                      const uint64_t* win_bytes, uint64_t schedule_seed, uint64_t* counters_out, uint64_t* direct_out,
                      uint64_t* steps_out) {
  if (!op_window && nops > 0) return -2;
  SimWindows T;
  T.nwin = nwin;
  T.base = win_base;
  T.bytes = win_bytes;
  static const int none = -1;
  return sim_p2p_run(n, channels, slots, slot_bytes, pipes, nphases, phase_coll, phase_sched, phase_count, csend, crecv, op,
                     nops, op_phase, op_rank, op_launch, op_send, op_peer, op_ptr, op_bytes, op_window ? op_window : &none, T,
                     schedule_seed, counters_out, direct_out, steps_out);
}

// the pure functions of p2p.h's window form, exported for the host-logic tests
int mnccl_p2p_win_slots(void) { return kP2pWinSlots; }
// ops[i] > 0: register window id ops[i]; < 0: deregister window -ops[i].  slots_out[i]: the slot taken or freed, -1: none
void mnccl_p2p_win_assign(int nops, const int64_t* ops, int* slots_out) {
  P2pWinSlots t;
  for (int i = 0; i < nops; ++i)
    slots_out[i] = ops[i] > 0 ? p2p_win_take(t, (uint64_t)ops[i]) : p2p_win_drop(t, (uint64_t)-ops[i]);
}
int mnccl_p2p_win_direct(int in_window, int slot, int device_memory) {
  return p2p_win_direct(in_window != 0, slot, device_memory != 0) ? 1 : 0;
}
// rec: tag, direct, slot, off, bytes -> words_out: info[0..2], tag -> back_out: the same five decoded
void mnccl_p2p_dest_roundtrip(const uint64_t* rec, uint64_t* words_out, uint64_t* back_out) {
  P2pDest d;
  d.tag = rec[0];
  d.direct = (uint32_t)rec[1];
  d.slot = (uint32_t)rec[2];
  d.off = rec[3];
  d.bytes = rec[4];
  p2p_dest_encode(d, words_out);
  words_out[kDestInfoWords] = d.tag;
  const P2pDest b = p2p_dest_decode(words_out, words_out[kDestInfoWords]);
  back_out[0] = b.tag; back_out[1] = b.direct; back_out[2] = b.slot; back_out[3] = b.off; back_out[4] = b.bytes;
}
uint64_t mnccl_p2p_dest_tag(uint64_t seq) { return p2p_dest_tag(seq); }
int mnccl_p2p_dest_check(int direct, uint32_t slot, uint64_t off, uint64_t bytes, uint64_t my_bytes, uint64_t win_base,
                         uint64_t win_bytes) {
  P2pDest d;
  d.tag = 1;
  d.direct = (uint32_t)direct;
  d.slot = slot;
  d.off = off;
  d.bytes = bytes;
  return p2p_dest_check(d, my_bytes, win_base, win_bytes);
}
uint64_t mnccl_mbox_word(int which, int n, int C, int q, int w) {
  return which == 0 ? mbox_ready(C, q, w) : which == 1 ? mbox_credit(n, C, q, w) : which == 2 ? mbox_abort(n, C)
         : which == 3 ? mbox_dest_info(n, C, q, w) : which == 4 ? mbox_dest_tag(n, C, q, w) : mbox_words(n, C);
}

// csrc/schedule.h one-shot geometry, exported for the host-logic tests
uint64_t mnccl_oneshot_slice(uint64_t chunk_bytes, int n, int channels, uint64_t slot_bytes) {
  return oneshot_slice(chunk_bytes, n, channels, slot_bytes);
}
int mnccl_oneshot_fits(uint64_t chunk_bytes, int n, int channels, uint64_t slot_bytes, int forced) {
  return oneshot_fits(chunk_bytes, n, channels, slot_bytes, forced != 0) ? 1 : 0;
}

// csrc/schedule.h op tables of the ring and its halves (coll_op; ring_op for comparison), exported
// for the host-logic tests: out = {kind, chunk, send_msg, recv_msg}
int mnccl_coll_num_ops(int coll, int n) { return coll_num_ops(coll, n); }
// ncclGather / ncclScatter: the op count of rank r with the call's root (their chains' depends on both)
int mnccl_coll_num_ops_at(int coll, int n, int r, int root) { return coll_num_ops(coll, n, r, root); }
int mnccl_coll_msgs_per_iter(int coll, int n) { return coll_msgs_per_iter(coll, n); }
// the same with a root (the rooted collectives' tables) and what each rank's counters advance by
void mnccl_coll_op_rooted(int coll, int n, int r, int k, int root, int* out) {
  const RingOp o = coll_op(coll, n, r, k, root);
  out[0] = o.kind; out[1] = o.chunk; out[2] = o.send_msg; out[3] = o.recv_msg;
}
int mnccl_coll_tx_msgs(int coll, int n, int r, int root) { return coll_tx_msgs(coll, n, r, root); }
int mnccl_coll_rx_msgs(int coll, int n, int r, int root) { return coll_rx_msgs(coll, n, r, root); }
uint64_t mnccl_rooted_len(uint64_t total_bytes, uint64_t chunk_off, uint64_t chunk_bytes, uint64_t slice_bytes, uint64_t s) {
  return rooted_len(total_bytes, chunk_off, chunk_bytes, slice_bytes, s);
}
void mnccl_coll_op(int coll, int n, int r, int k, int* out) {
  const RingOp o = coll < 0 ? ring_op(n, r, k) : coll_op(coll, n, r, k);  // coll < 0: ring_op itself
  out[0] = o.kind; out[1] = o.chunk; out[2] = o.send_msg; out[3] = o.recv_msg;
}

// csrc/schedule.h effective_slice, exported for the host-logic tests
uint64_t mnccl_effective_slice(uint64_t chunk_bytes, int channels, uint64_t slice, uint64_t min_slice, int depth) {
  return effective_slice(chunk_bytes, channels, slice, min_slice, depth);
}
// csrc/schedule.h pipeline_geometry (what Comm allocates and launches): out = {workgroups,
// waves, slot_bytes, scratch_bytes}
void mnccl_pipeline_geometry(int n, int channels, int threads, int window, int signal_batch, int slots,
                             uint64_t slice, uint64_t cap, uint64_t* out) {
  const Geometry g = pipeline_geometry(n, channels, threads, window, signal_batch, slots, slice, cap);
  out[0] = (uint64_t)g.workgroups;
  out[1] = (uint64_t)g.waves;
  out[2] = g.slot_bytes;
  out[3] = g.scratch_bytes;
}

uint64_t mnccl_read_slice(uint64_t chunk_bytes, int channels, uint64_t slice, uint64_t min_slice, int depth) {
  return read_slice(chunk_bytes, channels, slice, min_slice, depth);
}

int mnccl_call_pipelines(uint64_t nslices, int channels, int waves) { return call_pipelines(nslices, channels, waves); }
int mnccl_resident_pipes(int P, int waves, int cus, int most, int waves_per_simd) {
  return resident_pipes(P, waves, cus, most, waves_per_simd);
}

// schedule.h topology_blocks_read over an n x n matrix (rank q's row: how q's GPU reaches p's)
int mnccl_topology_blocks_read(int n, const int* link, const int* hops) { return topology_blocks_read(n, link, hops); }
int mnccl_read_grid_form(int forced, int auto_mode, int vec, uint64_t chunk_bytes, int n, uint64_t min_bytes) {
  return read_grid_form(forced != 0, auto_mode != 0, vec != 0, chunk_bytes, n, min_bytes) ? 1 : 0;
}
int mnccl_read_grid_vectors(int n) { return read_grid_vectors(n); }

// Runs `calls` consecutive all-reduces (send -> recv, fp32; send == recv for in place) on n
// simulated ranks with the GPU kernels' protocol; call i uses schedule (algo >> 3i) & 7 (0 ring,
// 1 one-shot, 2 read (persistent kernel), 4 read's grid form (3, the 4.0-5.x load form, is gone) -- START and
// DONE on pipeline 0, the whole chunk folded and pushed between them, as kernels.hip
// read_start / read_grid / read_done do; schedules can alternate on one communicator state, as
// mncclCommSetAlgo allows; at most 21 calls).  A one-shot call's slice: oneshot_slice when
// min_slice != 0 (Comm::launch; -2 if the call does not fit), else the slot.  schedule_seed != 0 permutes the order programs are tried
// in (pseudo-random), exploring different interleavings.  min_slice: 0 = fixed payload (the
// configured slice), else the adaptive payload of Comm::launch.  Returns 0, -1 on deadlock,
// -2 on bad arguments.  *steps_out = ops executed.
int mnccl_sim_allreduce(uint64_t algo, const float* const* send, float* const* recv, int n, uint64_t count, int op,
                        uint64_t slice_bytes, uint64_t min_slice, int channels, int slots, int calls,
                        uint64_t schedule_seed, uint64_t* steps_out) {
  if (n < 1 || n > 16 || channels < 1 || slots < 1 || slice_bytes < 4 || slice_bytes % 4) return -2;
  World W;
  init_world(W, n, channels, slots, op, slice_bytes);
  W.algo = (int)algo;
  uint64_t steps = 0;
  uint64_t rng = schedule_seed * 6364136223846793005ull + 1442695040888963407ull;
  for (int call = 0; call < calls; ++call) {
    const int rc = run_call(W, (int)((algo >> (3 * call)) & 7), kCollAllReduce, count, send, recv, slice_bytes, min_slice,
                            schedule_seed, rng, steps);
    if (rc != 0) return rc;
  }
  if (steps_out) *steps_out = steps;
  return 0;
}

// A sequence of calls of any collective on one simulated communicator state, as one communicator
// runs them: call i is collective coll[i] (schedule.h Coll: 0 all-reduce over counts[i] elements,
// 1 reduce-scatter / 2 all-gather of counts[i] elements per rank) on schedule sched[i] (the codes
// of mnccl_sim_allreduce; the halves have the ring and the persistent read form only), with rank
// r's buffers send[i * n + r] / recv[i * n + r] (in place as NCCL defines it; the tests size them).
// The other arguments and the return value as mnccl_sim_allreduce.
int mnccl_sim_collective(int n, int calls, const int* coll, const int* sched, const uint64_t* counts,
                         const float* const* send, float* const* recv, int op, uint64_t slice_bytes,
                         uint64_t min_slice, int channels, int slots, uint64_t schedule_seed, uint64_t* steps_out) {
  if (n < 1 || n > 16 || channels < 1 || slots < 1 || slice_bytes < 4 || slice_bytes % 4 || calls < 0) return -2;
  World W;
  init_world(W, n, channels, slots, op, slice_bytes);
  uint64_t steps = 0;
  uint64_t rng = schedule_seed * 6364136223846793005ull + 1442695040888963407ull;
  for (int call = 0; call < calls; ++call) {
    const int c = coll[call];
    if (c < kCollAllReduce || c > kCollAllGather || (c != kCollAllReduce && sched[call] != 0 && sched[call] != 2)) return -2;
    const int rc = run_call(W, sched[call], c, counts[call], send + (size_t)call * n, recv + (size_t)call * n, slice_bytes,
                            min_slice, schedule_seed, rng, steps);
    if (rc != 0) return rc;
  }
  if (steps_out) *steps_out = steps;
  return 0;
}

// mnccl_sim_collective with the two rooted collectives (schedule.h Coll 3 broadcast / 4 reduce over
// counts[i] elements) and a root per call, roots[i] (ignored by the other collectives): any of the
// five may follow any other, on either schedule, on the one communicator state.  A rank's unused
// buffer (a non-root's send / recv) may be NULL.
int mnccl_sim_rooted(int n, int calls, const int* coll, const int* sched, const uint64_t* counts, const int* roots,
                     const float* const* send, float* const* recv, int op, uint64_t slice_bytes, uint64_t min_slice,
                     int channels, int slots, uint64_t schedule_seed, uint64_t* steps_out) {
  if (n < 1 || n > 16 || channels < 1 || slots < 1 || slice_bytes < 4 || slice_bytes % 4 || calls < 0) return -2;
  World W;
  init_world(W, n, channels, slots, op, slice_bytes);
  uint64_t steps = 0;
  uint64_t rng = schedule_seed * 6364136223846793005ull + 1442695040888963407ull;
  for (int call = 0; call < calls; ++call) {
    const int c = coll[call];
    if (c < kCollAllReduce || c > kCollReduce || (c != kCollAllReduce && sched[call] != 0 && sched[call] != 2)) return -2;
    if (counts[call] == 0) return -2;
    const int rc = run_call(W, sched[call], c, counts[call], send + (size_t)call * n, recv + (size_t)call * n, slice_bytes,
                            min_slice, schedule_seed, rng, steps, roots[call]);
    if (rc != 0) return rc;
  }
  if (steps_out) *steps_out = steps;
  return 0;
}

// mnccl_sim_rooted with the all-to-all (schedule.h Coll 5: counts[i] elements per block, n blocks in
// both of a rank's buffers, which must not overlap): any of the six collectives may follow any
// other, on either schedule, on the one communicator state.
int mnccl_sim_mixed(int n, int calls, const int* coll, const int* sched, const uint64_t* counts, const int* roots,
                    const float* const* send, float* const* recv, int op, uint64_t slice_bytes, uint64_t min_slice,
                    int channels, int slots, uint64_t schedule_seed, uint64_t* steps_out) {
  if (n < 1 || n > 16 || channels < 1 || slots < 1 || slice_bytes < 4 || slice_bytes % 4 || calls < 0) return -2;
  World W;
  init_world(W, n, channels, slots, op, slice_bytes);
  uint64_t steps = 0;
  uint64_t rng = schedule_seed * 6364136223846793005ull + 1442695040888963407ull;
  for (int call = 0; call < calls; ++call) {
    const int c = coll[call];
    if (c < kCollAllReduce || c > kCollAllToAll || (c != kCollAllReduce && sched[call] != 0 && sched[call] != 2)) return -2;
    if (counts[call] == 0) return -2;
    const int rc = run_call(W, sched[call], c, counts[call], send + (size_t)call * n, recv + (size_t)call * n, slice_bytes,
                            min_slice, schedule_seed, rng, steps, roots[call]);
    if (rc != 0) return rc;
  }
  if (steps_out) *steps_out = steps;
  return 0;
}

// mnccl_sim_mixed with ncclAllToAllv (schedule.h Coll 6): any of the seven collectives may follow any
// other, on either schedule, on the one communicator state.  For a call of collective 6, counts[i] is
// ignored and vcounts / vsdispls / vrdispls + i * n * n hold the call's n x n matrices in elements of
// esz bytes ([r * n + q]: rank r's sendcounts[q] / sdispls[q] / rdispls[q]; recvcounts are the
// transpose -- the caller checks that with mnccl_varblock_matrix_mismatch); send / recv are bytes.
int mnccl_sim_varblock(int n, int calls, const int* coll, const int* sched, const uint64_t* counts, const int* roots,
                       const float* const* send, float* const* recv, int esz, const uint64_t* vcounts,
                       const uint64_t* vsdispls, const uint64_t* vrdispls, int op, uint64_t slice_bytes,
                       uint64_t min_slice, int channels, int slots, uint64_t schedule_seed, uint64_t* steps_out) {
  if (n < 1 || n > 16 || channels < 1 || slots < 1 || slice_bytes < 4 || slice_bytes % 4 || calls < 0) return -2;
  if (esz != 1 && esz != 2 && esz != 4 && esz != 8) return -2;
  World W;
  init_world(W, n, channels, slots, op, slice_bytes);
  uint64_t steps = 0;
  uint64_t rng = schedule_seed * 6364136223846793005ull + 1442695040888963407ull;
  for (int call = 0; call < calls; ++call) {
    const int c = coll[call];
    if (c < kCollAllReduce || c > kCollAllToAllV || (c != kCollAllReduce && sched[call] != 0 && sched[call] != 2)) return -2;
    int rc;
    if (c == kCollAllToAllV) {
      const size_t m = (size_t)call * n * n;
      rc = run_var_call(W, sched[call], esz, vcounts + m, vsdispls + m, vrdispls + m,
                        (const char* const*)(send + (size_t)call * n), (char* const*)(recv + (size_t)call * n), slice_bytes,
                        min_slice, schedule_seed, rng, steps);
    } else {
      if (counts[call] == 0) return -2;
      rc = run_call(W, sched[call], c, counts[call], send + (size_t)call * n, recv + (size_t)call * n, slice_bytes,
                    min_slice, schedule_seed, rng, steps, roots[call]);
    }
    if (rc != 0) return rc;
  }
  if (steps_out) *steps_out = steps;
  return 0;
}

// mnccl_sim_varblock with ncclGather / ncclScatter (schedule.h Coll 7 / 8: counts[i] elements per
// block; the root's large buffer -- Gather's recv, Scatter's send -- holds n blocks, every rank's other
// buffer one; a non-root's large buffer may be NULL and must stay untouched) and a root per call: all
// nine collectives may follow one another, on either schedule, on the one communicator state.  The
// variable all-to-all's matrices may be NULL when no call is one.
int mnccl_sim_all_collectives(int n, int calls, const int* coll, const int* sched, const uint64_t* counts, const int* roots,
                              const float* const* send, float* const* recv, int esz, const uint64_t* vcounts,
                              const uint64_t* vsdispls, const uint64_t* vrdispls, int op, uint64_t slice_bytes,
                              uint64_t min_slice, int channels, int slots, uint64_t schedule_seed, uint64_t* steps_out) {
  if (n < 1 || n > 16 || channels < 1 || slots < 1 || slice_bytes < 4 || slice_bytes % 4 || calls < 0) return -2;
  if (esz != 1 && esz != 2 && esz != 4 && esz != 8) return -2;
  World W;
  init_world(W, n, channels, slots, op, slice_bytes);
  uint64_t steps = 0;
  uint64_t rng = schedule_seed * 6364136223846793005ull + 1442695040888963407ull;
  for (int call = 0; call < calls; ++call) {
    const int c = coll[call];
    if (c < kCollAllReduce || c > kCollScatter || (c != kCollAllReduce && sched[call] != 0 && sched[call] != 2)) return -2;
    int rc;
    if (c == kCollAllToAllV) {
      if (!vcounts || !vsdispls || !vrdispls) return -2;
      const size_t m = (size_t)call * n * n;
      rc = run_var_call(W, sched[call], esz, vcounts + m, vsdispls + m, vrdispls + m,
                        (const char* const*)(send + (size_t)call * n), (char* const*)(recv + (size_t)call * n), slice_bytes,
                        min_slice, schedule_seed, rng, steps);
    } else {
      if (counts[call] == 0) return -2;
      rc = run_call(W, sched[call], c, counts[call], send + (size_t)call * n, recv + (size_t)call * n, slice_bytes,
                    min_slice, schedule_seed, rng, steps, roots[call]);
    }
    if (rc != 0) return rc;
  }
  if (steps_out) *steps_out = steps;
  return 0;
}

// mnccl_sim_all_collectives' eight collectives with uniform counts (every Coll but ncclAllToAllv) and
// mncclAllGatherv / mncclReduceScatterv (schedule.h Coll 9 / 10), in any order, on either schedule, on
// the one communicator state.  For a call of collective 9 / 10, counts[i] is ignored and vcounts /
// vdispls + i * n hold the call's n counts and displacements in elements (of esz bytes for the gather,
// of 4 for the fold: fp32), the same on every rank; send[i * n + r] / recv[i * n + r] are rank r's
// sendbuff / recvbuff as the C call takes them (the one-block buffer may be NULL where counts[r] is 0).
int mnccl_sim_vhalves(int n, int calls, const int* coll, const int* sched, const uint64_t* counts, const int* roots,
                      const float* const* send, float* const* recv, int esz, const uint64_t* vcounts,
                      const uint64_t* vdispls, int op, uint64_t slice_bytes, uint64_t min_slice, int channels, int slots,
                      uint64_t schedule_seed, uint64_t* steps_out) {
  if (n < 1 || n > 16 || channels < 1 || slots < 1 || slice_bytes < 4 || slice_bytes % 4 || calls < 0) return -2;
  if (esz != 1 && esz != 2 && esz != 4 && esz != 8) return -2;
  World W;
  init_world(W, n, channels, slots, op, slice_bytes);
  uint64_t steps = 0;
  uint64_t rng = schedule_seed * 6364136223846793005ull + 1442695040888963407ull;
  for (int call = 0; call < calls; ++call) {
    const int c = coll[call];
    if (c < kCollAllReduce || c > kCollReduceScatterV || c == kCollAllToAllV) return -2;
    if (c != kCollAllReduce && sched[call] != 0 && sched[call] != 2) return -2;
    int rc;
    if (c == kCollAllGatherV || c == kCollReduceScatterV) {
      if (!vcounts || !vdispls) return -2;
      char* const* s = (char* const*)(send + (size_t)call * n);
      char* const* r = (char* const*)(recv + (size_t)call * n);
      rc = run_vhalf_call(W, sched[call], c, c == kCollAllGatherV ? esz : 4, vcounts + (size_t)call * n,
                          vdispls + (size_t)call * n, c == kCollAllGatherV ? r : s, c == kCollAllGatherV ? s : r, slice_bytes,
                          min_slice, schedule_seed, rng, steps);
    } else {
      if (counts[call] == 0) return -2;
      rc = run_call(W, sched[call], c, counts[call], send + (size_t)call * n, recv + (size_t)call * n, slice_bytes,
                    min_slice, schedule_seed, rng, steps, roots[call]);
    }
    if (rc != 0) return rc;
  }
  if (steps_out) *steps_out = steps;
  return 0;
}

// One read call (push form) on registered windows: every rank's START carries sigs[r] and every
// pipeline compares its peers' with its own before touching data (kernels.hip starts_agree).
// mismatch_out[r] = pipelines of rank r that gave up.  0: every pipeline ran; 1: some gave up
// (then every pipeline must have, and no recv touched); -1 deadlock; -2 bad arguments.
int mnccl_sim_signed_read(const float* const* send, float* const* recv, int n, uint64_t count, int channels,
                          uint64_t slice_bytes, const uint64_t* sigs, uint64_t schedule_seed, int* mismatch_out) {
  if (n < 2 || n > 16 || channels < 1 || slice_bytes < 4 || slice_bytes % 4) return -2;
  World W;
  W.n = n; W.C = channels; W.K = 2; W.op = 0; W.algo = 2; W.slot_bytes = slice_bytes;
  W.chunk_bytes = count / (uint64_t)n * 4;
  W.send.assign(send, send + n);
  W.recv.assign(recv, recv + n);
  W.mbox.assign((size_t)n, std::vector<uint64_t>((size_t)mbox_words(n, channels), 0));
  W.tx_seq.assign((size_t)n, std::vector<uint64_t>((size_t)n * channels, 0));
  W.rx_seq.assign((size_t)n, std::vector<uint64_t>((size_t)n * channels, 0));
  W.sig.assign(sigs, sigs + n);
  W.mismatch.assign((size_t)n, 0);
  W.slice = slice_bytes;
  W.nslices = (W.chunk_bytes + W.slice - 1) / W.slice;
  W.A = call_pipelines(W.nslices, channels, 1);
  W.iters = (uint32_t)((W.nslices + (uint64_t)W.A - 1) / (uint64_t)W.A);
  if (W.chunk_bytes == 0) return -2;
  std::vector<Prog> progs;
  for (int r = 0; r < n; ++r)
    for (int w = 0; w < W.A; ++w) {
      Prog p;
      p.r = r; p.w = w;
      progs.push_back(p);
    }
  uint64_t rng = schedule_seed * 6364136223846793005ull + 1442695040888963407ull;
  for (;;) {
    bool any = false, all_done = true;
    const size_t np = progs.size();
    rng = rng * 6364136223846793005ull + 1442695040888963407ull;
    const size_t start = (size_t)((rng >> 33) % np);
    for (size_t j = 0; j < np; ++j) {
      Prog& P = progs[(start + j) % np];
      if (P.done) continue;
      all_done = false;
      rng = rng * 6364136223846793005ull + 1442695040888963407ull;
      const int burst = 1 + (int)((rng >> 40) % 4);
      for (int b = 0; b < burst && !P.done; ++b) {
        if (!read_step(W, P)) break;
        any = true;
      }
    }
    if (all_done) break;
    if (!any) return -1;
  }
  int total = 0;
  for (int r = 0; r < n; ++r) {
    mismatch_out[r] = W.mismatch[r];
    total += W.mismatch[r];
  }
  return total ? 1 : 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------
// Host-only hooks for the CPU test suite: the bootstrap (TCP star) and the env config,
// exercised without a GPU.  Not part of libmini_nccl.so.
#include <stdio.h>

#include <stdexcept>
#include <string>
#include <thread>

#include <unistd.h>

#include "bootstrap.h"
#include "config.h"
#include "kernels.h"
#include "peerbuf.h"
#include "split.h"

extern "C" {

// connect, all-gather a 256-byte record per rank, barrier twice; 0 on success,
// -1 on exception, -2 if gathered contents are wrong.
int mnccl_bootstrap_selftest(int rank, int nranks, const char* ip, int port, int timeout_ms) {
  try {
    mnccl::Bootstrap b;
    b.connect(rank, nranks, ip ? ip : "127.0.0.1", port, timeout_ms / 1000.0);
    unsigned char mine[256];
    for (int i = 0; i < 256; ++i) mine[i] = (unsigned char)(rank * 31 + i);
    std::vector<unsigned char> all((size_t)nranks * 256);
    b.allgather(mine, all.data(), 256);
    b.barrier();
    for (int r = 0; r < nranks; ++r)
      for (int i = 0; i < 256; ++i)
        if (all[(size_t)r * 256 + i] != (unsigned char)(r * 31 + i)) return -2;
    b.barrier();
    return 0;
  } catch (const std::exception& e) {
    fprintf(stderr, "bootstrap selftest rank %d: %s\n", rank, e.what());
    return -1;
  }
}

// The read schedule's per-call rendezvous (csrc/peerbuf.cpp) across real processes, without a
// GPU: every call is negotiated with eligible = false (host buffers), so no HIP call is made
// and the decision must be kFallback on every rank -- except where the ranks disagree on the
// count (scenario 1: call calls/2 -> kMismatch everywhere) or one rank never calls (scenario 2:
// the others time out).  Scenario 3 adds random host delays per rank (the 16-record board
// wraps around many times).  decisions[i] = PeerBuffers::Decision of call i, -9 on timeout.
// Returns 0, -1 on an unexpected exception, -3 without shared memory.
int mnccl_board_selftest(int rank, int nranks, const char* ip, int port, int scenario, int calls,
                         double timeout_s, int* decisions) {
  try {
    mnccl::Bootstrap b;
    b.connect(rank, nranks, ip ? ip : "127.0.0.1", port, 20.0);
    std::vector<uint64_t> nonces((size_t)nranks);
    for (int q = 0; q < nranks; ++q) nonces[(size_t)q] = 1000u + (uint64_t)q;  // one process per rank
    mnccl::PeerBuffers pb;
    // scenario 7: the last rank's descriptor socket is out of its peers' reach (another network
    // namespace): init must turn the read schedule off on EVERY rank (-3), within seconds
    if (scenario == 7 && rank == nranks - 1) pb.set_test_unreachable(true);
    pb.init(b, rank, nranks, nonces, port);
    if (!pb.available()) return -3;
    // scenarios 4 / 5: every rank eligible with synthetic buffers (no HIP); 4: rank 1 cannot map
    // on call 3 (every rank must fall back on that call alone); 5: the same buffers every call
    // after the first (the mapping round runs once), except a fresh buffer on call calls/2
    // scenario 6: as 5, and at call calls/2 every rank reports its first buffers freed (its
    // peers close their mappings of them, every rank forgets them)
    std::vector<char> arena(1 << 20);
    const bool fake = scenario == 4 || scenario == 5 || scenario == 6;
    if (fake) pb.set_test_fake(true, scenario == 4 && rank == 1 ? 3u : 0u);
    uint64_t rng = 0x9E3779B97F4A7C15ull * (uint64_t)(rank + 1);
    for (int i = 0; i < calls; ++i) decisions[i] = 99;
    for (int i = 0; i < calls; ++i) {
      if (scenario == 2 && rank == nranks - 1) break;  // this rank never reaches the calls
      if (scenario == 3) {
        rng = rng * 6364136223846793005ull + 1442695040888963407ull;
        usleep((useconds_t)((rng >> 33) % 300));
      }
      const uint64_t count = (scenario == 1 && i == calls / 2) ? 1000u + (uint64_t)rank : 1000u;
      const char* ps[mnccl::kMaxRanks] = {};
      const char* pr[mnccl::kMaxRanks] = {};
      bool vec = false;
      try {
        const void* sb = nullptr;
        void* rb = nullptr;
        if (scenario == 4) {  // a new send / recv page every call
          sb = arena.data() + (size_t)(2 * i) * 4096 % arena.size();
          rb = arena.data() + (size_t)(2 * i + 1) * 4096 % arena.size();
        } else if (scenario == 5 || scenario == 6) {
          const int gen = scenario == 6 ? (i >= calls / 2 ? 1 : 0) : i == calls / 2 ? 1 : 0;
          if (scenario == 6 && i == calls / 2)
            for (int g = 0; g < 2; ++g) {
              const char* p = arena.data() + (size_t)g * 4096;
              pb.test_report_freed((uint64_t)(uintptr_t)p & ~(uint64_t)4095, (uint64_t)(uintptr_t)p);
            }
          sb = arena.data() + (size_t)(2 * gen) * 4096;
          rb = arena.data() + (size_t)(2 * gen + 1) * 4096;
        }
        decisions[i] = (int)pb.negotiate(sb, rb, fake, count, 7, 0, timeout_s, [] {}, ps, pr, &vec);
        if (fake) decisions[i] += 10 * (int)pb.agreements();  // decision + 10 x mapping rounds so far
        if (scenario == 6) decisions[i] += 1000 * (int)pb.closed_freed();  // + 1000 x mappings closed
      } catch (const std::runtime_error&) {
        decisions[i] = -9;
        break;
      }
    }
    b.barrier();
    return 0;
  } catch (const std::exception& e) {
    fprintf(stderr, "board selftest rank %d: %s\n", rank, e.what());
    return -1;
  }
}

// csrc/varblock.h, the host-side rules of ncclAllToAllv, for the CPU suite: one rank's local checks
// (a VarLocal verdict; the buffers are only compared, never dereferenced) and the matrix check on
// n x n counts ([r * n + q]; 0, or 1 + r * n + q of the first pair that differs)
int mnccl_varblock_check_local(int n, int esz, const void* send, const size_t* sendcounts, const size_t* sdispls,
                               const void* recv, const size_t* recvcounts, const size_t* rdispls) {
  if (n < 1 || n > mnccl::kVarMaxRanks || esz < 1) return -2;
  return mnccl::varblock_check_local(n, esz, send, sendcounts, sdispls, recv, recvcounts, rdispls);
}
int mnccl_varblock_matrix_mismatch(int n, const uint64_t* sendcounts, const uint64_t* recvcounts) {
  if (n < 1 || n > mnccl::kVarMaxRanks) return -2;
  mnccl::VarRow rows[mnccl::kVarMaxRanks];
  memset(rows, 0, sizeof rows);
  for (int r = 0; r < n; ++r)
    for (int q = 0; q < n; ++q) {
      rows[r].sendcounts[q] = sendcounts[(size_t)r * n + q];
      rows[r].recvcounts[q] = recvcounts[(size_t)r * n + q];
    }
  return mnccl::varblock_matrix_mismatch(n, rows);
}
uint64_t mnccl_varblock_len(uint64_t block_bytes, uint64_t slice_bytes, uint64_t s) {
  return mnccl::varblock_len(block_bytes, slice_bytes, s);
}

// csrc/vhalves.h, the host-side rules of mncclAllGatherv / mncclReduceScatterv, and schedule.h's length
// rule for them.  mnccl_vhalf_rows_differ: counts / displs are n x n, row r what rank r passed.
int mnccl_vhalf_check_local(int n, int rank, int esz, const void* array_buf, const size_t* counts, const size_t* displs,
                            const void* one_buf, size_t one_count) {
  return mnccl::vhalf_check_local(n, rank, esz, array_buf, counts, displs, one_buf, one_count);
}
int mnccl_vhalf_rows_differ(int n, const uint64_t* counts, const uint64_t* displs) {
  if (n < 1 || n > mnccl::kVarMaxRanks) return -1;
  mnccl::VarRow rows[mnccl::kVarMaxRanks];
  memset(rows, 0, sizeof rows);
  for (int r = 0; r < n; ++r)
    for (int q = 0; q < n; ++q) {
      rows[r].sendcounts[q] = counts[(size_t)r * n + q];
      rows[r].rdispls[q] = displs[(size_t)r * n + q];
    }
  return mnccl::vhalf_rows_differ(n, rows);
}
uint64_t mnccl_vhalf_len(uint64_t block_bytes, uint64_t slice_bytes, uint64_t s) {
  return mnccl::vhalf_len(block_bytes, slice_bytes, s);
}
int mnccl_vhalf_vec(int vec_all, uint64_t base_bytes, uint64_t block_bytes) {
  return mnccl::vhalf_vec(vec_all != 0, base_bytes, block_bytes) ? 1 : 0;
}

// Config::from_env() rendered to text; -1 if the environment is invalid.
int mnccl_config_describe(char* buf, int len) {
  try {
    const std::string s = mnccl::Config::from_env().describe();
    snprintf(buf, (size_t)len, "%s", s.c_str());
    return 0;
  } catch (const std::exception& e) {
    snprintf(buf, (size_t)len, "%s", e.what());
    return -1;
  }
}

// ncclCommSplit's plan (csrc/split.h split_plan): out[3 * r] = {group size, new rank, leader's parent
// rank} of rank r, {0, -1, -1} for a rank in no group.
void mnccl_split_plan(int n, const int* colors, const int* keys, int* out) {
  std::vector<mnccl::SplitSlot> plan((size_t)(n > 0 ? n : 0));
  mnccl::split_plan(n, colors, keys, plan.data());
  for (int r = 0; r < n; ++r) {
    out[3 * r] = plan[(size_t)r].size;
    out[3 * r + 1] = plan[(size_t)r].rank;
    out[3 * r + 2] = plan[(size_t)r].leader;
  }
}

}  // extern "C"

// One rank of mnccl_bootstrap_split_selftest: a split of `parent` by (color, key), then on the child
// star one all-gather of the members' parent ranks -- which must come back in the plan's order --
// and one barrier.  0, or -2 wrong slot, -3 wrong gathered order, -4 a socket where none is due.
static int split_round(mnccl::Bootstrap& parent, int n, const int* colors, const int* keys, double timeout_s) {
  const int me = parent.rank();
  std::vector<mnccl::SplitSlot> plan((size_t)n);
  mnccl::split_plan(n, colors, keys, plan.data());
  mnccl::Bootstrap child;
  int port = -1;
  const mnccl::SplitSlot s = mnccl::split_bootstrap(parent, colors[me], keys[me], timeout_s, &child, &port);
  const mnccl::SplitSlot want = plan[(size_t)me];
  if (s.size != want.size || s.rank != want.rank || s.leader != want.leader) return -2;
  if (s.size == 0) return child.nranks() == 0 && port == 0 ? 0 : -4;
  if (child.rank() != s.rank || child.nranks() != s.size || (s.size == 1) != (port == 0)) return -4;
  const int32_t mine = me;
  std::vector<int32_t> all((size_t)s.size, -1);
  child.allgather(&mine, all.data(), sizeof mine);
  child.barrier();
  for (int q = 0; q < n; ++q)
    if (plan[(size_t)q].size > 0 && plan[(size_t)q].leader == s.leader && all[(size_t)plan[(size_t)q].rank] != q) return -3;
  return 0;
}

extern "C" {

// The two-round bootstrap of ncclCommSplit (csrc/bootstrap.h split_bootstrap) with n ranks as threads
// of this process over 127.0.0.1:port: the parent star connects, splits by (colors, keys), every
// child star runs split_round's all-gather and barrier, then the parent star all-gathers again (it
// still works), splits a second time with the keys negated (every group in reverse order), and runs
// a last barrier.  0 on success, -1 an exception, -5 the parent's all-gather came back wrong, or the
// first failing rank's split_round code.
int mnccl_bootstrap_split_selftest(int n, int port, const int* colors, const int* keys, int timeout_ms) {
  if (n < 1 || n > 64) return -1;
  const double timeout_s = timeout_ms / 1000.0;
  std::vector<int> rcs((size_t)n, 0), neg((size_t)n);
  for (int r = 0; r < n; ++r) neg[(size_t)r] = -keys[r];
  auto rank_main = [&](int r) {
    try {
      mnccl::Bootstrap parent;
      parent.connect(r, n, "127.0.0.1", port, timeout_s);
      int rc = split_round(parent, n, colors, keys, timeout_s);
      const int32_t mine = 100 + r;
      std::vector<int32_t> all((size_t)n, -1);
      parent.allgather(&mine, all.data(), sizeof mine);
      for (int q = 0; q < n && rc == 0; ++q)
        if (all[(size_t)q] != 100 + q) rc = -5;
      if (rc == 0) rc = split_round(parent, n, colors, neg.data(), timeout_s);
      parent.barrier();
      rcs[(size_t)r] = rc;
    } catch (const std::exception& e) {
      fprintf(stderr, "bootstrap split selftest rank %d: %s\n", r, e.what());
      rcs[(size_t)r] = -1;
    }
  };
  std::vector<std::thread> ts;
  for (int r = 0; r < n; ++r) ts.emplace_back(rank_main, r);
  for (auto& t : ts) t.join();
  for (int rc : rcs)
    if (rc != 0) return rc;
  return 0;
}

}  // extern "C"
