// combinemx.h -- the host-side rules of mncclAllToAllvCombineMxfp8 (mncclAllToAllvCombine whose send
// side holds MXFP8 records, the layout mncclAllToAllvRowsMxfp8 delivers), as pure functions: no HIP, no
// communicator.  Comm::combine applies them, kernels.hip (combinemx_fold, combinemx_local) reads the
// same CombineArgs as the plain combine, and the simulator exports all of it to the CPU suite.
//
// Row i of `send` is one record of P = rowcount + rowcount / 32 bytes (mxblock.h): rowcount e4m3
// elements, then one E8M0 scale byte per 32 consecutive elements.  Counts, displacements and slotidx
// are in records.  The recv side is combine.h's matrix of bf16 / fp16 / f32 rows; `datatype` and
// `rowstride` are ITS.  The fold is combine.h's with float(P[j][e]) replaced by the decoded element:
// NaN when the scale byte is 0xFF or the code is 0x7F / 0xFF, else e4m3(code) * 2^(scale - 127) in
// IEEE single -- exact wherever it is representable (every scale the dispatch writes, subnormal
// results included), +-inf for scale bytes 247 .. 254 where it is not.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "combine.h"
#include "mxblock.h"

namespace mnccl {

// One rank's arguments; esz: the OUTPUT element size.  mxblock.h's two verdicts first (kMxRowcount,
// kMxAlign), then combine_check_local's in its order with P bytes per send row.
inline int combinemx_check_local(int n, int esz, const void* send, const size_t* sendcounts, const size_t* sdispls,
                                 const void* recv, size_t nrows, size_t rowstride, const int32_t* slotidx,
                                 const float* weights, int topk, const size_t* recvcounts, const size_t* rdispls,
                                 size_t rowcount) {
  if (rowcount % kMxRowMultiple || rowcount < kMxRowMultiple || rowcount > kMxMaxRowcount) return kMxRowcount;
  if (((uint64_t)(uintptr_t)send | (uint64_t)(uintptr_t)recv | (uint64_t)rowstride * (uint64_t)esz) % 4) return kMxAlign;
  return combine_check_local(n, esz, send, sendcounts, sdispls, recv, nrows, rowstride, slotidx, weights, topk, recvcounts,
                             rdispls, rowcount, mx_record_bytes(rowcount));
}

// CombineArgs of the call: row_bytes is the OUTPUT row's (the kernels derive rowcount = row_bytes / esz
// and P from it), src_off[q] the byte offset of the block's first RECORD in rank q's send
inline void combinemx_fill_args(CombineArgs* v, int n, int esz, const void* recv, size_t nrows, size_t rowstride,
                                const int32_t* slotidx, const float* weights, int topk, const size_t* recvcounts,
                                const size_t* rdispls, size_t rowcount, const void* const* send_of,
                                const uint64_t* peer_sdispl) {
  combine_fill_args(v, n, esz, recv, nrows, rowstride, slotidx, weights, topk, recvcounts, rdispls, rowcount, send_of,
                    peer_sdispl);
  for (int q = 0; q < n; ++q) v->src_off[q] = peer_sdispl[q] * mx_record_bytes(rowcount);
}

// ---------------------------------------------------------------- the host decoder (the simulator's)
// an e4m3 code as a float: exact (0x7F / 0xFF: NaN)
inline float mx_decode_e4m3(uint8_t c) {
  const uint32_t e = (c >> 3) & 15u, m = c & 7u;
  if ((c & 0x7fu) == 0x7fu) return NAN;
  const float a = e ? ldexpf((float)(8u + m), (int)e - 10) : ldexpf((float)m, -9);
  return c & 0x80u ? -a : a;
}

// element `e` of a record: the mirror of mx_quantise_row (ldexpf is exact where the result is
// representable, rounds to +-inf above FLT_MAX)
inline float mx_decode_elem(const uint8_t* rec, uint32_t rowcount, uint32_t e) {
  const uint8_t c = rec[e], s = rec[rowcount + e / kMxBlock];
  if (s == 0xffu || (c & 0x7fu) == 0x7fu) return NAN;
  return ldexpf(mx_decode_e4m3(c), (int)s - 127);
}

// One output row before its rounding to the datatype: acc = +0, then for every slot in order whose
// position lies in [0, nrec) of the packed sequence `recs`, one single multiply and one single add
inline void combinemx_fold_row(const uint8_t* recs, uint64_t nrec, uint32_t rowcount, const int32_t* slots,
                               const float* weights, int topk, float* out) {
  const uint64_t P = mx_record_bytes(rowcount);
  for (uint32_t e = 0; e < rowcount; ++e) {
    volatile float acc = 0.0f;  // (volatile: a product and a sum, never a fused one)
    for (int k = 0; k < topk; ++k) {
      if (slots[k] < 0 || (uint64_t)slots[k] >= nrec) continue;
      volatile float prod = (weights ? weights[k] : 1.0f) * mx_decode_elem(recs + (uint64_t)slots[k] * P, rowcount, e);
      acc = acc + prod;
    }
    out[e] = acc;
  }
}

}  // namespace mnccl
