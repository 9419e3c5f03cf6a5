// vhalves.h -- the host-side rules of mncclAllGatherv / mncclReduceScatterv (the all-reduce's halves
// with per-rank counts and displacements), as pure functions: no HIP, no communicator.  Comm::vhalf
// applies them, the rendezvous (peerbuf.h) carries the rows, and the simulator library exports them
// so the CPU suite can call them on hand-made cases.
//
// Both calls have an ARRAY side -- mncclAllGatherv's recv, mncclReduceScatterv's send: n blocks, block
// q at elements [displs[q], displs[q] + counts[q]) -- and a SCALAR side, the one block of this rank
// (mncclAllGatherv's send, mncclReduceScatterv's recv) of `one_count` elements.  A call is valid when
// one_count == counts[rank], a NULL buffer goes with zero counts on its side, nothing overflows, the
// non-empty blocks of the array side do not overlap each other (an in-place mncclReduceScatterv writes
// block `rank` of a buffer whose other blocks the peers are reading), the scalar side is either block
// `rank` itself (in place) or overlaps no non-empty block, and counts / displs are the same arrays
// on every rank: one byte offset then serves every peer's buffer.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "varblock.h"

namespace mnccl {

// The local checks' verdicts, in the order they are made
enum VHalfLocal : int {
  kVHalfOk = 0,
  kVHalfCountMismatch = 1,  // the scalar count differs from counts[rank]
  kVHalfNullBuffer = 2,     // a NULL buffer on a side that has a non-zero count
  kVHalfOverflow = 3,       // displ + count, a byte size or an address overflows size_t
  kVHalfBlockOverlap = 4,   // two non-empty blocks of the array side overlap
  kVHalfScalarOverlap = 5   // the scalar-side buffer overlaps a non-empty block and is not in place
};

// One rank's arguments.  esz: the element size in bytes; counts / displs hold n entries.
inline int vhalf_check_local(int n, int rank, int esz, const void* array_buf, const size_t* counts, const size_t* displs,
                             const void* one_buf, size_t one_count) {
  if (one_count != counts[rank]) return kVHalfCountMismatch;
  bool any = false;
  for (int q = 0; q < n; ++q) any = any || counts[q] != 0;
  if ((any && !array_buf) || (one_count && !one_buf)) return kVHalfNullBuffer;
  const uint64_t e = (uint64_t)esz, top = ~(uint64_t)0;
  const uint64_t base = (uint64_t)(uintptr_t)array_buf, one = (uint64_t)(uintptr_t)one_buf;
  uint64_t b[kVarMaxRanks], l[kVarMaxRanks];  // byte ranges of the non-empty blocks, as addresses
  for (int q = 0; q < n; ++q) {
    const uint64_t c = counts[q], d = displs[q];
    b[q] = l[q] = 0;
    if (c == 0) continue;  // an empty block's displacement is never used
    if (d > top - c || d + c > top / e || base > top - (d + c) * e) return kVHalfOverflow;
    b[q] = base + d * e;
    l[q] = c * e;
  }
  if (one_count && (one_count > top / e || one > top - one_count * e)) return kVHalfOverflow;
  for (int q = 0; q < n; ++q)
    for (int p = q + 1; p < n; ++p)
      if (l[q] && l[p] && var_ranges_overlap(b[q], l[q], b[p], l[p])) return kVHalfBlockOverlap;
  if (one_count && one != b[rank])  // (one == b[rank]: in place, and block `rank` overlaps no other)
    for (int q = 0; q < n; ++q)
      if (l[q] && var_ranges_overlap(one, one_count * e, b[q], l[q])) return kVHalfScalarOverlap;
  return kVHalfOk;
}

// What a rank publishes for one call is a VarRow (varblock.h) with counts in `sendcounts`, displs in
// `rdispls`, `recvcounts` zero and kVarSameRows set: the rendezvous then compares the rows for
// equality instead of transposition.  0 when every rank's counts and displs equal rank 0's, else
// 1 + r * n + q of the first entry that differs.  Every rank runs it on the same rows.
inline int vhalf_rows_differ(int n, const VarRow* rows) {
  for (int r = 1; r < n; ++r)
    for (int q = 0; q < n; ++q)
      if (rows[r].sendcounts[q] != rows[0].sendcounts[q] || rows[r].rdispls[q] != rows[0].rdispls[q]) return 1 + r * n + q;
  return 0;
}

// The largest block in elements: the call's geometry follows it (the same on every rank)
inline uint64_t vhalf_max_count(int n, const VarRow& row) {
  uint64_t m = 0;
  for (int q = 0; q < n; ++q) m = row.sendcounts[q] > m ? row.sendcounts[q] : m;
  return m;
}

// The 16-byte path of one rank (kernels.hip vhalf_fold / vhalf_push): every rank's buffers are
// dword-aligned (the rendezvous' vec_all), and so are this rank's block base and length in bytes.
// Ranks of one call may differ in it: the protocol counts messages by the call's iterations alone.
inline bool vhalf_vec(bool vec_all, uint64_t base_bytes, uint64_t block_bytes) {
  return vec_all && base_bytes % 4 == 0 && block_bytes % 4 == 0;
}

}  // namespace mnccl
