// varblock.h -- the host-side rules of ncclAllToAllv (all-to-all with per-peer counts and
// displacements), as pure functions: no HIP, no communicator.  Comm::all_to_all_v applies them, the
// rendezvous (peerbuf.h) carries the rows, and the simulator library exports them so the CPU suite
// can call them on hand-made cases.
//
// Elements [sdispls[q], sdispls[q] + sendcounts[q]) of rank r's send become elements
// [rdispls[r], rdispls[r] + recvcounts[r]) of rank q's recv.  A call is valid when, on every rank,
// the non-empty recv blocks overlap neither each other nor a non-empty send block (send blocks may
// overlap each other: they are only read), nothing overflows, a NULL buffer goes with all-zero
// counts, and sendcounts_r[q] == recvcounts_q[r] for every pair.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace mnccl {

constexpr int kVarMaxRanks = 16;  // kernels.h kMaxRanks

// What a rank publishes for one ncclAllToAllv call: every rank reads every row, so every rank sees
// the whole n x n matrix and reaches the same verdict.  sdispls stays private to the rank.
struct VarRow {
  uint64_t sendcounts[kVarMaxRanks], recvcounts[kVarMaxRanks], rdispls[kVarMaxRanks];  // elements
  uint32_t flags;  // kVarCapturing
  uint32_t pad;
};
enum : uint32_t {
  kVarCapturing = 1u,  // this rank's stream is being captured into a graph
  // the row of an mncclAllGatherv / mncclReduceScatterv call (vhalves.h): counts in sendcounts, displs
  // in rdispls; the ranks' rows must be EQUAL, where ncclAllToAllv's must be each other's transpose
  kVarSameRows = 2u
};

// The local checks' verdicts, in the order they are made
enum VarLocal : int {
  kVarOk = 0,
  kVarNullBuffer = 1,    // a NULL sendbuff / recvbuff with a non-zero count on that side
  kVarOverflow = 2,      // displ + count, a byte size or an address overflows size_t
  kVarRecvOverlap = 3,   // two non-empty recv blocks overlap
  kVarSendRecvOverlap = 4  // a non-empty recv block overlaps a non-empty send block
};

// [a, a + la) and [b, b + lb) overlap (both non-empty, neither end overflows: checked before)
inline bool var_ranges_overlap(uint64_t a, uint64_t la, uint64_t b, uint64_t lb) { return a < b + lb && b < a + la; }

// One rank's arguments.  esz: the element size in bytes; the arrays hold n entries.
inline int varblock_check_local(int n, int esz, const void* send, const size_t* sendcounts, const size_t* sdispls,
                                const void* recv, const size_t* recvcounts, const size_t* rdispls) {
  bool any_s = false, any_r = false;
  for (int q = 0; q < n; ++q) {
    any_s = any_s || sendcounts[q] != 0;
    any_r = any_r || recvcounts[q] != 0;
  }
  if ((any_s && !send) || (any_r && !recv)) return kVarNullBuffer;
  const uint64_t e = (uint64_t)esz, top = ~(uint64_t)0;
  // byte ranges of the non-empty blocks, as addresses
  uint64_t sb[kVarMaxRanks], sl[kVarMaxRanks], rb[kVarMaxRanks], rl[kVarMaxRanks];
  for (int side = 0; side < 2; ++side) {
    const uint64_t base = (uint64_t)(uintptr_t)(side ? recv : send);
    const size_t* counts = side ? recvcounts : sendcounts;
    const size_t* displs = side ? rdispls : sdispls;
    for (int q = 0; q < n; ++q) {
      const uint64_t c = counts[q], d = displs[q];
      (side ? rl : sl)[q] = 0;
      (side ? rb : sb)[q] = 0;
      if (c == 0) continue;  // an empty block's displacement is never used
      if (d > top - c || d + c > top / e || base > top - (d + c) * e) return kVarOverflow;
      (side ? rb : sb)[q] = base + d * e;
      (side ? rl : sl)[q] = c * e;
    }
  }
  for (int q = 0; q < n; ++q)
    for (int p = q + 1; p < n; ++p)
      if (rl[q] && rl[p] && var_ranges_overlap(rb[q], rl[q], rb[p], rl[p])) return kVarRecvOverlap;
  for (int q = 0; q < n; ++q)
    for (int p = 0; p < n; ++p)
      if (rl[q] && sl[p] && var_ranges_overlap(rb[q], rl[q], sb[p], sl[p])) return kVarSendRecvOverlap;
  return kVarOk;
}

// The matrix check: 0 when sendcounts_r[q] == recvcounts_q[r] for every pair, else 1 + r * n + q of
// the first pair that differs.  Every rank runs it on the same rows.
inline int varblock_matrix_mismatch(int n, const VarRow* rows) {
  for (int r = 0; r < n; ++r)
    for (int q = 0; q < n; ++q)
      if (rows[r].sendcounts[q] != rows[q].recvcounts[r]) return 1 + r * n + q;
  return 0;
}

// The largest block of the matrix in elements: the call's geometry follows it (the same on every rank)
inline uint64_t varblock_max_count(int n, const VarRow* rows) {
  uint64_t m = 0;
  for (int r = 0; r < n; ++r)
    for (int q = 0; q < n; ++q) m = rows[r].sendcounts[q] > m ? rows[r].sendcounts[q] : m;
  return m;
}

// Some rank's stream is capturing: the padded fallback (which may allocate its stage) is refused
inline bool varblock_any_capturing(int n, const VarRow* rows) {
  for (int r = 0; r < n; ++r)
    if (rows[r].flags & kVarCapturing) return true;
  return false;
}

}  // namespace mnccl
