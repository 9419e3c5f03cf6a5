// p2p.h -- the host-side bookkeeping of ncclSend / ncclRecv / ncclGroupStart / ncclGroupEnd, as pure
// functions: no HIP, no communicator.  api.cpp keeps one P2pGroup per thread and records into it,
// Comm::p2p_group builds the kernel's second argument from it (kernels.hip p2p_kernel), and the
// simulator (sim.cpp mnccl_sim_p2p) runs the same builder, so the wave-per-(pair, pipeline) mapping
// the CPU suite checks is the one the GPU executes.  Compiles into a stand-alone program
// (tests/native/p2p_selftest.cpp).  The second half of the file is the zero-copy form on registered
// windows (kernels.hip p2p_window_group, sim.cpp mnccl_sim_p2p_win): the window table's slots, the
// per-recv direct / scratch decision, and the DEST record with the sender's check of it.
//
// A group is a list of operations in call order.  A directed pair is (direction, peer): the sends
// to one peer, or the recvs from one peer.  The operations of a pair run in call order on that
// pair's pipelines; different pairs never share a wave.  A send to the own rank pairs with a recv
// from the own rank, in order, and becomes one device copy inside the launch.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "schedule.h"

namespace mnccl {

constexpr int kMaxGroupOps = 64;  // operations per group: fits the by-value kernel argument
constexpr int kP2pMaxPairs = 32;  // >= 2 (kMaxRanks - 1) directed pairs

// The verdicts of the checks, in the order they are made
enum P2pVerdict : int {
  kP2pOk = 0,
  kP2pPeerRange = 1,     // peer outside [0, nranks): ncclInvalidArgument
  kP2pOverflow = 2,      // count * element size, or the buffer's end, overflows size_t: ncclInvalidArgument
  kP2pOverlap = 3,       // a recv range overlaps another recv range or a send range of the group: ncclInvalidArgument
  kP2pTooMany = 4,       // more than kMaxGroupOps operations: ncclInvalidUsage
  kP2pSelfUngrouped = 5, // peer == rank outside a group: ncclInvalidUsage
  kP2pSelfUnpaired = 6,  // a self send without a self recv, or the reverse, at ncclGroupEnd: ncclInvalidUsage
  kP2pSelfSize = 7       // a self send and its recv differ in bytes: ncclInvalidUsage
};

struct P2pOp {
  int32_t send;    // 1 send, 0 recv
  int32_t peer;
  uint64_t addr;   // the caller's pointer (overlap checks)
  uint64_t kaddr;  // the address the kernel uses (a pinned host buffer's device mapping)
  uint64_t bytes;
};

struct P2pGroup {
  int32_t nops = 0;
  P2pOp ops[kMaxGroupOps];
};

// [a, a + la) and [b, b + lb) overlap (both non-empty, neither end overflows: checked before)
inline bool p2p_ranges_overlap(uint64_t a, uint64_t la, uint64_t b, uint64_t lb) { return a < b + lb && b < a + la; }

// One operation against the group recorded so far (count != 0; the caller made the NULL, count == 0
// and datatype checks): the peer's range, the byte size, the overlaps.  *bytes_out: count * esz.
inline int p2p_check_op(const P2pGroup& g, int nranks, bool send, int peer, const void* buf, size_t count, int esz,
                        uint64_t* bytes_out) {
  if (peer < 0 || peer >= nranks) return kP2pPeerRange;
  const uint64_t top = ~(uint64_t)0, e = (uint64_t)esz, a = (uint64_t)(uintptr_t)buf;
  if ((uint64_t)count > top / e || a > top - (uint64_t)count * e) return kP2pOverflow;
  const uint64_t b = (uint64_t)count * e;
  for (int i = 0; i < g.nops; ++i) {
    const P2pOp& o = g.ops[i];
    // send ranges may overlap each other: they are only read
    if ((send && o.send) || !p2p_ranges_overlap(a, b, o.addr, o.bytes)) continue;
    return kP2pOverlap;
  }
  *bytes_out = b;
  return kP2pOk;
}

// Appends a checked operation (kaddr: where the kernel reaches the buffer)
inline int p2p_append(P2pGroup& g, bool send, int peer, const void* buf, uint64_t kaddr, uint64_t bytes) {
  if (g.nops >= kMaxGroupOps) return kP2pTooMany;
  P2pOp& o = g.ops[g.nops++];
  o.send = send ? 1 : 0;
  o.peer = peer;
  o.addr = (uint64_t)(uintptr_t)buf;
  o.kaddr = kaddr;
  o.bytes = bytes;
  return kP2pOk;
}

// The kernel's second argument (by value, as VarBlockArgs): the operations sorted by directed pair
// -- pairs in order of first appearance, a pair's operations in call order -- then the self copies
// as (source, destination) entry pairs.  Wave b of the launch serves pair b / pipes on pipeline
// b % pipes; the waves from npairs * pipes on copy the self pairs.
struct P2pArgs {
  uint64_t ptr[kMaxGroupOps];    // this rank's buffer of the operation (kernel-addressable)
  uint64_t bytes[kMaxGroupOps];  // the message's bytes
  uint8_t vec[kMaxGroupOps];     // 16-byte path: the pointer is dword-aligned (this end's choice alone)
  uint8_t pair_peer[kP2pMaxPairs], pair_send[kP2pMaxPairs], pair_first[kP2pMaxPairs], pair_count[kP2pMaxPairs];
  int32_t npairs;      // directed pairs with a peer in this launch
  int32_t pipes;       // waves per pair in this launch: the most pipelines one of its messages uses
  int32_t p2p_pipes;   // schedule.h p2p_pipes: what a message's pipelines are cut for (rank-uniform)
  int32_t nself;       // self copies: entries self_first + 2k (source) and + 2k + 1 (destination)
  int32_t self_first;
  int32_t self_waves;  // waves that copy them (0 when nself == 0)
  int32_t pad[2];
};

constexpr uint64_t kP2pSelfWaveBytes = 64u << 10;  // one self-copy wave per this many bytes,
constexpr int kP2pMaxSelfWaves = 32;               // up to this many

// Builds the argument from a group of checked operations: self pairing, pair ordering, the launch's
// width.  kP2pOk, kP2pSelfUnpaired or kP2pSelfSize.
inline int p2p_build(const P2pGroup& g, int rank, int pipes_per_msg, uint64_t slot_bytes, P2pArgs* out) {
  P2pArgs& a = *out;
  memset(&a, 0, sizeof a);
  a.p2p_pipes = pipes_per_msg;
  int at = 0;
  bool placed[kMaxGroupOps] = {};
  for (int i = 0; i < g.nops; ++i) {
    if (placed[i] || g.ops[i].peer == rank) continue;
    // a new directed pair: every operation of it, in call order
    const int p = a.npairs++;
    a.pair_peer[p] = (uint8_t)g.ops[i].peer;
    a.pair_send[p] = (uint8_t)g.ops[i].send;
    a.pair_first[p] = (uint8_t)at;
    for (int j = i; j < g.nops; ++j) {
      const P2pOp& o = g.ops[j];
      if (placed[j] || o.peer != g.ops[i].peer || o.send != g.ops[i].send) continue;
      placed[j] = true;
      a.ptr[at] = o.kaddr;
      a.bytes[at] = o.bytes;
      a.vec[at] = (uint8_t)(o.kaddr % 4 == 0 && slot_bytes % 4 == 0);
      const int A = p2p_msg_pipes(o.bytes, slot_bytes, pipes_per_msg);
      if (A > a.pipes) a.pipes = A;
      ++at;
    }
    a.pair_count[p] = (uint8_t)(at - a.pair_first[p]);
  }
  // the self pair: the k-th send to the own rank with the k-th recv from it
  a.self_first = at;
  uint64_t self_bytes = 0;
  int s = 0, r = 0;
  for (;;) {
    while (s < g.nops && !(g.ops[s].peer == rank && g.ops[s].send)) ++s;
    while (r < g.nops && !(g.ops[r].peer == rank && !g.ops[r].send)) ++r;
    if (s >= g.nops && r >= g.nops) break;
    if (s >= g.nops || r >= g.nops) return kP2pSelfUnpaired;
    if (g.ops[s].bytes != g.ops[r].bytes) return kP2pSelfSize;
    a.ptr[at] = g.ops[s].kaddr;
    a.ptr[at + 1] = g.ops[r].kaddr;
    a.bytes[at] = a.bytes[at + 1] = g.ops[s].bytes;
    a.vec[at] = a.vec[at + 1] = (uint8_t)((g.ops[s].kaddr | g.ops[r].kaddr) % 4 == 0);
    self_bytes += g.ops[s].bytes;
    at += 2;
    ++a.nself;
    ++s;
    ++r;
  }
  if (a.nself) {
    const uint64_t want = (self_bytes + kP2pSelfWaveBytes - 1) / kP2pSelfWaveBytes;
    a.self_waves = want < 1 ? 1 : want > (uint64_t)kP2pMaxSelfWaves ? kP2pMaxSelfWaves : (int)want;
  }
  return kP2pOk;
}

// waves of the launch (0: nothing to launch)
inline int p2p_launch_waves(const P2pArgs& a) { return a.npairs * a.pipes + a.self_waves; }

// ---- the zero-copy form on registered windows (kernels.hip p2p_window_group) ----
// On a communicator with at least one registered window the receiver of every message tells its
// sender, from the device, where the bytes go: straight into the recv buffer when that lies in a
// window (the sender has every window mapped since the collective registration), else into the
// scratch as before.  Everything the two kernels and the simulator share is here.

// The communicator's window table: slot s holds one registered window -- this rank's mapping of
// every rank's buffer of it and the window's byte size (the same on every rank).  Slots are assigned
// identically on every rank (registration is collective and ordered): the lowest free one.  A window
// registered while the table is full has no slot, and recvs into it are posted "scratch".
constexpr int kP2pWinSlots = 16;
constexpr int kP2pNoSlot = 0xff;  // P2pWinArgs::wslot of an entry that is posted "scratch"

struct P2pWinSlots {
  uint64_t id[kP2pWinSlots] = {};  // the window's registration number, 0: free
};
// the lowest free slot for window `id` (!= 0), or -1 when the table is full
inline int p2p_win_take(P2pWinSlots& t, uint64_t id) {
  for (int s = 0; s < kP2pWinSlots; ++s)
    if (t.id[s] == 0) {
      t.id[s] = id;
      return s;
    }
  return -1;
}
inline int p2p_win_find(const P2pWinSlots& t, uint64_t id) {
  for (int s = 0; s < kP2pWinSlots; ++s)
    if (id != 0 && t.id[s] == id) return s;
  return -1;
}
// frees the slot of window `id`; -1 when it had none
inline int p2p_win_drop(P2pWinSlots& t, uint64_t id) {
  const int s = p2p_win_find(t, id);
  if (s >= 0) t.id[s] = 0;
  return s;
}

// The table as the kernel reads it (device memory of the communicator; the host uploads base and
// bytes after every registration and deregistration, once the previous call has completed).
struct P2pWinTable {
  uint64_t base[kP2pWinSlots][16];  // [slot][rank]: rank's buffer of the window, mapped here (0: free slot)
  uint64_t bytes[kP2pWinSlots];     // the window's size
  uint64_t direct_sends[16];        // per peer: messages this rank's kernels pushed direct (device-owned)
};

// Whether a recv is posted direct: its range lies in a window (Comm::find_window) that has a table
// slot, and the buffer is device memory (a pinned host buffer goes through the scratch).
inline bool p2p_win_direct(bool in_window, int slot, bool device_memory) {
  return in_window && device_memory && slot >= 0 && slot < kP2pWinSlots;
}

// The DEST record a receiver posts per message (schedule.h mbox_dest_info / mbox_dest_tag).
struct P2pDest {
  uint64_t tag;     // the pair's message counter on this pipeline at the message's start + 1: full width
  uint32_t direct;  // 1: push into window `slot` at byte `off`; 0: into the scratch
  uint32_t slot;
  uint64_t off;
  uint64_t bytes;   // the receiver's byte count of the message, on both paths
};
MNCCL_HD uint64_t p2p_dest_tag(uint64_t seq) { return seq + 1; }
// info[kDestInfoWords]: kind and slot, offset, bytes
MNCCL_HD void p2p_dest_encode(const P2pDest& d, uint64_t* info) {
  info[0] = (uint64_t)(d.direct ? 1u : 0u) | ((uint64_t)d.slot << 8);
  info[1] = d.off;
  info[2] = d.bytes;
}
MNCCL_HD P2pDest p2p_dest_decode(const uint64_t* info, uint64_t tag) {
  P2pDest d;
  d.tag = tag;
  d.direct = (uint32_t)(info[0] & 1u);
  d.slot = (uint32_t)(info[0] >> 8);
  d.off = info[1];
  d.bytes = info[2];
  return d;
}
// The sender's check of a record before it stores anything.  win_base / win_bytes: the sender's
// table entry for (d.slot, the receiver), read only when d.slot < kP2pWinSlots.
enum P2pDestVerdict : int {
  kDestOk = 0,
  kDestBytes = 1,  // the posted byte count differs from the sender's (both paths)
  kDestSlot = 2,   // the window slot is out of range or free on this rank
  kDestRange = 3   // offset + bytes does not lie inside the window
};
MNCCL_HD int p2p_dest_check(const P2pDest& d, uint64_t my_bytes, uint64_t win_base, uint64_t win_bytes) {
  if (d.bytes != my_bytes) return kDestBytes;
  if (!d.direct) return kDestOk;
  if (d.slot >= (uint32_t)kP2pWinSlots || win_base == 0) return kDestSlot;
  if (d.off > win_bytes || d.bytes > win_bytes - d.off) return kDestRange;
  return kDestOk;
}

// The window kernel's second argument: the old one, and per entry of a.ptr what a recv posts.
struct P2pWinArgs {
  P2pArgs a;
  uint64_t woff[kMaxGroupOps];   // a direct recv's byte offset in its window
  uint8_t wslot[kMaxGroupOps];   // its window's table slot, kP2pNoSlot: the recv is posted "scratch"
  P2pWinTable* table;            // the communicator's table (device)
  uint64_t* host_sends;          // host-mapped mirror of table->direct_sends (16 words)
};

// Builds it: p2p_build, then op_slot[j] / op_off[j] of group operation j (a recv the caller decided
// to post direct: p2p_win_direct; anything else kP2pNoSlot) moved to the operation's entry.  Entry
// pair_first[p] + k is the k-th operation of pair p in call order.
inline int p2p_win_build(const P2pGroup& g, int rank, int pipes_per_msg, uint64_t slot_bytes, const uint8_t* op_slot,
                         const uint64_t* op_off, P2pWinArgs* out) {
  memset(out, 0, sizeof *out);
  const int v = p2p_build(g, rank, pipes_per_msg, slot_bytes, &out->a);
  memset(out->wslot, kP2pNoSlot, sizeof out->wslot);
  if (v != kP2pOk) return v;
  const P2pArgs& a = out->a;
  for (int p = 0; p < a.npairs; ++p) {
    int at = a.pair_first[p];
    for (int j = 0; j < g.nops; ++j) {
      const P2pOp& o = g.ops[j];
      if (o.peer == rank || o.peer != a.pair_peer[p] || o.send != a.pair_send[p]) continue;
      if (!o.send && op_slot[j] < kP2pWinSlots) {
        out->wslot[at] = op_slot[j];
        out->woff[at] = op_off[j];
      }
      ++at;
    }
  }
  return kP2pOk;
}

}  // namespace mnccl
