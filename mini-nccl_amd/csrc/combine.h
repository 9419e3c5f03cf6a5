// combine.h -- the host-side rules of mncclAllToAllvCombine (the way back of a mixture-of-experts
// layer: ncclAllToAllv whose packed recv is never built, because the token owner folds the up to
// top-k returned rows of each token, each times its gate weight, into one output row), as pure
// functions: no HIP, no communicator.  Comm::combine applies them, the rendezvous carries the rows
// (varblock.h VarRow with kVarCombine), kernels.hip (combine_fold, combine_local) reads CombineArgs,
// and the simulator library exports all of it so the CPU suite can call it on hand-made cases.
//
// The send side is dense: the block for rank q is rows [sdispls[q], + sendcounts[q]) of `send`, rows
// of `rowcount` elements.  On rank r the VIRTUAL packed sequence P has P[rdispls[q] + i] = row
// sdispls_q[r] + i of rank q's send, i < recvcounts[q] -- what ncclAllToAllv would deliver.  The recv
// side is a matrix of `nrows` rows, row t at element t * rowstride; y[t] = sum over k < topk, in that
// order, of weights[t * topk + k] * P[slotidx[t * topk + k]], in float, rounded once.  A slot whose
// index lies in no non-empty block contributes nothing.  The slices of the read schedule are cut out
// of the output rows' packed sequence by rowblock.h rows_units, unchanged.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "rowblock.h"

namespace mnccl {

constexpr int kCombineMaxTopk = 16;

// The local checks' verdicts, in the order they are made
enum CombineLocal : int {
  kCombineOk = 0,
  kCombineTopk = 1,            // topk outside [1, 16]
  kCombineZeroRow = 2,         // rowcount == 0 with a non-zero count or nrows
  kCombineStride = 3,          // rowstride < rowcount
  kCombineTooManySlots = 4,    // nrows * topk > INT32_MAX
  kCombineNullBuffer = 5,      // a NULL send with a non-zero sendcount; a NULL recv / slotidx with nrows > 0
  kCombineOverflow = 6,        // a size or an address overflows (a row of 2 GiB or more counts as that)
  kCombineRecvOverlap = 7,     // two non-empty blocks of the virtual sequence overlap
  kCombineSendRecvOverlap = 8  // the recv matrix's byte extent overlaps a non-empty send block, slotidx or weights
};

// One rank's arguments.  esz: the element size in bytes; the arrays hold n entries.  The buffers are
// only compared, never dereferenced.  send_row_bytes: the bytes of one row of `send` where they are not
// rowcount * esz (combinemx.h: a record), else 0.
inline int combine_check_local(int n, int esz, const void* send, const size_t* sendcounts, const size_t* sdispls,
                               const void* recv, size_t nrows, size_t rowstride, const int32_t* slotidx,
                               const float* weights, int topk, const size_t* recvcounts, const size_t* rdispls,
                               size_t rowcount, uint64_t send_row_bytes = 0) {
  bool any_s = false, any_r = false;
  for (int q = 0; q < n; ++q) {
    any_s = any_s || sendcounts[q] != 0;
    any_r = any_r || recvcounts[q] != 0;
  }
  if (topk < 1 || topk > kCombineMaxTopk) return kCombineTopk;
  if (rowcount == 0 && (any_s || any_r || nrows != 0)) return kCombineZeroRow;
  if (rowstride < rowcount) return kCombineStride;
  if (nrows > (size_t)INT32_MAX / (size_t)topk) return kCombineTooManySlots;
  if ((any_s && !send) || (nrows != 0 && (!recv || !slotidx))) return kCombineNullBuffer;
  const uint64_t e = (uint64_t)esz, top = ~(uint64_t)0;
  if (rowcount > (uint64_t)INT32_MAX / e) return kCombineOverflow;
  const uint64_t rb = rowcount * e, srb = send_row_bytes ? send_row_bytes : rb;
  // the send blocks as address ranges; the virtual blocks as ranges of positions
  uint64_t sb[kVarMaxRanks] = {}, sl[kVarMaxRanks] = {};
  const uint64_t sbase = (uint64_t)(uintptr_t)send;
  for (int q = 0; q < n; ++q) {
    const uint64_t c = sendcounts[q], d = sdispls[q];
    if (c == 0) continue;  // an empty block's displacement is never used
    if (d > top - c || d + c > top / srb || sbase > top - (d + c) * srb) return kCombineOverflow;
    sb[q] = sbase + d * srb;
    sl[q] = c * srb;
  }
  for (int q = 0; q < n; ++q)
    if (recvcounts[q] && rdispls[q] > top - recvcounts[q]) return kCombineOverflow;
  for (int q = 0; q < n; ++q)
    for (int p = q + 1; p < n; ++p)
      if (recvcounts[q] && recvcounts[p] && var_ranges_overlap(rdispls[q], recvcounts[q], rdispls[p], recvcounts[p]))
        return kCombineRecvOverlap;
  if (nrows == 0) return kCombineOk;  // nothing is written: recv, slotidx and weights are not used
  if (rowstride > top / e || (nrows - 1) > (top - rb) / (rowstride * e)) return kCombineOverflow;
  const uint64_t ext = rows_extent_bytes(nrows, rowstride, rowcount, esz), rbase = (uint64_t)(uintptr_t)recv;
  const uint64_t slots = (uint64_t)nrows * (uint64_t)topk * 4, ibase = (uint64_t)(uintptr_t)slotidx,
                 wbase = (uint64_t)(uintptr_t)weights;
  if (rbase > top - ext || ibase > top - slots || (weights && wbase > top - slots)) return kCombineOverflow;
  for (int q = 0; q < n; ++q)
    if (sl[q] && var_ranges_overlap(rbase, ext, sb[q], sl[q])) return kCombineSendRecvOverlap;
  if (var_ranges_overlap(rbase, ext, ibase, slots)) return kCombineSendRecvOverlap;
  if (weights && var_ranges_overlap(rbase, ext, wbase, slots)) return kCombineSendRecvOverlap;
  return kCombineOk;
}

// ---------------------------------------------------------------- the kernels' view
// The second by-value kernel argument of combine_fold and combine_local.  Indexed by source rank q;
// this rank's own block at [rank].  combine_local reads one packed buffer: one range over all of it.
struct CombineArgs {
  const int32_t* slotidx;  // device-readable; read when the kernel runs
  const float* weights;    // the same, or nullptr: every weight 1
  uint64_t stride_bytes;   // rowstride * element size
  uint32_t row_bytes;      // rowcount * element size (< 2 GiB)
  uint32_t nrows;          // output rows of this rank
  uint32_t topk;
  uint32_t vec;            // 1: the 16-byte path (combine_vec_ok)
  uint64_t lo[16];         // rdispls[q]: the block's first position of the virtual sequence
  uint64_t cnt[16];        // recvcounts[q] (0: positions of q's range are in no block)
  uint64_t src_off[16];    // byte offset of the block's first row in rank q's send (rank q's sdispls[rank] * row_bytes)
};

// The 16-byte path: every source the call reads, the own recv, the stride and the row are dword-aligned
inline bool combine_vec_ok(int n, const void* const* send_of, const uint64_t* cnt, const void* recv, uint64_t stride_bytes,
                           uint64_t row_bytes) {
  uint64_t bits = (uint64_t)(uintptr_t)recv | stride_bytes | row_bytes;
  for (int q = 0; q < n; ++q)
    if (cnt[q]) bits |= (uint64_t)(uintptr_t)send_of[q];
  return bits % 4 == 0;
}

// send_of[q]: this rank's address of rank q's send; peer_sdispl[q]: rank q's sdispls[rank], in rows
inline void combine_fill_args(CombineArgs* v, int n, int esz, const void* recv, size_t nrows, size_t rowstride,
                              const int32_t* slotidx, const float* weights, int topk, const size_t* recvcounts,
                              const size_t* rdispls, size_t rowcount, const void* const* send_of,
                              const uint64_t* peer_sdispl) {
  *v = CombineArgs{};
  v->slotidx = slotidx;
  v->weights = weights;
  v->stride_bytes = (uint64_t)rowstride * (uint64_t)esz;
  v->row_bytes = (uint32_t)(rowcount * (size_t)esz);
  v->nrows = (uint32_t)nrows;
  v->topk = (uint32_t)topk;
  for (int q = 0; q < n; ++q) {
    v->lo[q] = rdispls[q];
    v->cnt[q] = recvcounts[q];
    v->src_off[q] = peer_sdispl[q] * (uint64_t)v->row_bytes;
  }
  v->vec = combine_vec_ok(n, send_of, v->cnt, recv, v->stride_bytes, v->row_bytes) ? 1u : 0u;
}

// The owner of position j of the virtual sequence: the rank q whose non-empty block holds it, else -1
// (negative positions, positions beyond or between the blocks).  What the kernels' scan computes.
MNCCL_HD int combine_owner(const CombineArgs& v, int n, int32_t j) {
  int own = -1;
  for (int q = 0; q < n; ++q)
    if (j >= 0 && (uint64_t)j >= v.lo[q] && (uint64_t)j - v.lo[q] < v.cnt[q]) own = q;
  return own;
}

// The call's geometry: the longest output matrix of any rank, in bytes of packed rows (the same on
// every rank, which is why every rank's nrows rides in the rendezvous)
inline uint64_t combine_max_rows(int n, const VarRow* rows) {
  uint64_t m = 0;
  for (int r = 0; r < n; ++r) m = rows[r].nrows > m ? rows[r].nrows : m;
  return m;
}

}  // namespace mnccl
