// combinefp8b.h -- the host-side rules of mncclAllToAllvCombineFp8Block128 (mncclAllToAllvCombine whose
// send side holds the "1 x 128" FP8 records mncclAllToAllvRowsFp8Block128 delivers), as pure functions:
// no HIP, no communicator.  Comm::combine applies them, kernels.hip (combinefp8b_fold, combinefp8b_local)
// reads the same CombineArgs as the plain combine, and the simulator exports all of it to the CPU suite.
//
// Row i of `send` is one record of P = rowcount + rowcount / 32 bytes (fp8block.h): rowcount e4m3
// elements, then rowcount / 128 little-endian IEEE singles, one per 128 consecutive elements.  Counts,
// displacements and slotidx are in records.  The recv side is combine.h's matrix of bf16 / fp16 / f32
// rows; `datatype` and `rowstride` are ITS.  The fold is combine.h's with float(P[j][e]) replaced by the
// decoded element d: a NaN when the code is 0x7F / 0xFF, else round_f32(e4m3(code) * S) with S the
// block's single as its bits say -- ONE IEEE multiply, denormals honoured, nothing special-cased, so a
// NaN S gives NaN, an infinite S +-inf (NaN against a zero code), a negative S flips the sign and a
// zero or subnormal S acts as IEEE says.  Then w * d and the add, each rounded, never fused.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "combine.h"
#include "combinemx.h"
#include "fp8block.h"

namespace mnccl {

// One rank's arguments; esz: the OUTPUT element size.  mxblock.h's two verdicts first (kMxRowcount,
// kMxAlign), then combine_check_local's in its order with P bytes per send row.
inline int combinefp8b_check_local(int n, int esz, const void* send, const size_t* sendcounts, const size_t* sdispls,
                                   const void* recv, size_t nrows, size_t rowstride, const int32_t* slotidx,
                                   const float* weights, int topk, const size_t* recvcounts, const size_t* rdispls,
                                   size_t rowcount) {
  if (rowcount % kMxRowMultiple || rowcount < kMxRowMultiple || rowcount > kMxMaxRowcount) return kMxRowcount;
  if (((uint64_t)(uintptr_t)send | (uint64_t)(uintptr_t)recv | (uint64_t)rowstride * (uint64_t)esz) % 4) return kMxAlign;
  return combine_check_local(n, esz, send, sendcounts, sdispls, recv, nrows, rowstride, slotidx, weights, topk, recvcounts,
                             rdispls, rowcount, fp8b_record_bytes(rowcount));
}

// CombineArgs of the call: row_bytes is the OUTPUT row's (the kernels derive rowcount = row_bytes / esz
// and P from it), src_off[q] the byte offset of the block's first RECORD in rank q's send
inline void combinefp8b_fill_args(CombineArgs* v, int n, int esz, const void* recv, size_t nrows, size_t rowstride,
                                  const int32_t* slotidx, const float* weights, int topk, const size_t* recvcounts,
                                  const size_t* rdispls, size_t rowcount, const void* const* send_of,
                                  const uint64_t* peer_sdispl) {
  combine_fill_args(v, n, esz, recv, nrows, rowstride, slotidx, weights, topk, recvcounts, rdispls, rowcount, send_of,
                    peer_sdispl);
  for (int q = 0; q < n; ++q) v->src_off[q] = peer_sdispl[q] * fp8b_record_bytes(rowcount);
}

// ---------------------------------------------------------------- the host decoder (the simulator's)
// element `e` of a record; volatile: the product is one single multiply as written, whatever the flags
inline float fp8b_decode_elem(const uint8_t* rec, uint32_t rowcount, uint32_t e) {
  uint32_t word = 0;
  for (uint32_t k = 0; k < 4; ++k) word |= (uint32_t)rec[rowcount + 4 * (e / kFp8bBlock) + k] << (8 * k);  // little-endian
  float s;
  memcpy(&s, &word, 4);
  volatile float d = mx_decode_e4m3(rec[e]) * s;
  return d;
}

// One output row before its rounding to the datatype: acc = +0, then for every slot in order whose
// position lies in [0, nrec) of the packed sequence `recs`, one single multiply and one single add
inline void combinefp8b_fold_row(const uint8_t* recs, uint64_t nrec, uint32_t rowcount, const int32_t* slots,
                                 const float* weights, int topk, float* out) {
  const uint64_t P = fp8b_record_bytes(rowcount);
  for (uint32_t e = 0; e < rowcount; ++e) {
    volatile float acc = 0.0f;  // (volatile: a product and a sum, never a fused one)
    for (int k = 0; k < topk; ++k) {
      if (slots[k] < 0 || (uint64_t)slots[k] >= nrec) continue;
      volatile float prod = (weights ? weights[k] : 1.0f) * fp8b_decode_elem(recs + (uint64_t)slots[k] * P, rowcount, e);
      acc = acc + prod;
    }
    out[e] = acc;
  }
}

}  // namespace mnccl
