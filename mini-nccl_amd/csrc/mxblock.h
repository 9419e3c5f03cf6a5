// mxblock.h -- the rules of mncclAllToAllvRowsMxfp8 (mncclAllToAllvRows whose rows are quantised to
// MXFP8 on the way out), as pure functions: no HIP, no communicator.  Comm::var_exchange applies the
// local checks, kernels.hip (rowsmx_push, rowsmx_pack) and the simulator share the record and scale
// rules, and the simulator exports all of it, with a host quantiser of one row, to the CPU suite.
//
// The send side is rowblock.h's: a strided matrix of bf16 / fp16 rows named by a device-side index
// list.  Each delivered row is one RECORD of P = rowcount + rowcount / 32 bytes: rowcount e4m3
// elements, then one E8M0 scale byte per block of 32 consecutive elements.  Counts and displacements
// of the receive side are in records.
//
// The rule, per block of 32 elements widened exactly to f32: E = the largest biased exponent field
// of the 32 magnitudes.  E == 255 (a NaN or an infinity): scale 0xFF, every element 0x7F.  Else the
// scale byte is s = max(E - 8, 0) and element x becomes encode_e4m3(x * 2^(127 - s)): exact scaling,
// one rounding to nearest even, finite overflow saturated to +-448, the sign of zero kept.
//
// mncclAllToAllvRowsMxfp4 (the mx4_ names; kernels.hip rowsmx4_push, rowsmx4_pack) is the same call with
// e2m1 elements, two to a byte: a record is P4 = rowcount / 2 + rowcount / 32 bytes, element 2i in the
// low nibble of byte i and element 2i + 1 in the high one, then the scale bytes.  E == 255: scale 0xFF,
// every element byte 0x77 (+6, +6).  Else s = max(E - 2, 0) and element x becomes the code of
// x * 2^(127 - s) on the grid {0, 0.5, 1, 1.5, 2, 3, 4, 6}: exact scaling, one rounding to nearest, ties
// to the even code, magnitudes above 6 saturated to 6, the sign kept (0x8 is -0).  The slice rule, the
// local checks and the kernels' argument block are the ones below, with P4 for P.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "rowblock.h"
#include "schedule.h"

namespace mnccl {

constexpr uint32_t kMxBlock = 32;           // elements per scale byte
constexpr uint32_t kMxRowMultiple = 128;    // records and their scale parts are whole dwords
constexpr uint32_t kMxMaxRowcount = 16384;  // 512 scale bytes: the kernels' per-wave LDS strip
constexpr uint32_t kMxPassElems = 1024;     // elements a wave quantises per pass: 16 per lane

constexpr uint32_t kMx4PassElems = 2048;    // the same for MXFP4: 32 per lane, a block per lane

// bytes of one record
MNCCL_HD uint64_t mx_record_bytes(uint64_t rowcount) { return rowcount + rowcount / kMxBlock; }
MNCCL_HD uint64_t mx4_record_bytes(uint64_t rowcount) { return rowcount / 2 + rowcount / kMxBlock; }

// the E8M0 scale byte of a block whose largest magnitude has f32 exponent field E
MNCCL_HD uint32_t mx_scale_byte(uint32_t E) { return E == 255u ? 255u : E > 8u ? E - 8u : 0u; }
MNCCL_HD uint32_t mx4_scale_byte(uint32_t E) { return E == 255u ? 255u : E > 2u ? E - 2u : 0u; }

// The slice rule.  A block is the virtual packed sequence of its records and the call's slices are
// cut for the largest block (varblock_len_at), so slice [a, b) may begin and end inside a record.  A
// record belongs to the slice that holds its FIRST byte and travels whole with it -- rowblock.h's
// straddling-vector rule taken to the record: no row is quantised twice, no amax is computed from a
// partial row, and every byte of the block is stored exactly once.  The records of [a, b): [*j0, *j1).
MNCCL_HD void mx_slice_records(uint64_t a, uint64_t b, uint64_t P, uint64_t* j0, uint64_t* j1) {
  *j0 = (a + P - 1) / P;
  *j1 = (b + P - 1) / P;
}

// The local checks' verdicts beyond rowblock.h's, in the order they are made (ahead of RowsLocal's)
enum MxLocal : int {
  kMxRowcount = 16,  // rowcount % 128 != 0, or outside [128, 16384]
  kMxAlign = 17      // sendbuff, rowstride in bytes, or recvbuff not dword-aligned
};

// One rank's arguments; esz: the SEND element size (2); P: the record's bytes (mx_record_bytes or
// mx4_record_bytes of rowcount).  The receive side gets rows_check_local's overlap, overflow and NULL
// checks with P for the row's bytes: the check is made twice, once per side.
inline int mx_check_local(int n, int esz, const void* send, size_t nrows, size_t rowstride, const int32_t* rowidx,
                          const size_t* sendcounts, const size_t* sdispls, const void* recv, const size_t* recvcounts,
                          const size_t* rdispls, size_t rowcount, uint64_t P) {
  if (rowcount % kMxRowMultiple || rowcount < kMxRowMultiple || rowcount > kMxMaxRowcount) return kMxRowcount;
  if (((uint64_t)(uintptr_t)send | (uint64_t)(uintptr_t)recv | (uint64_t)rowstride * (uint64_t)esz) % 4) return kMxAlign;
  if (rowstride < rowcount) return kRowsStride;
  // the send side as it is, against a recv side that cannot collide (checked below with the record's bytes)
  const size_t none[kVarMaxRanks] = {};
  int rc = rows_check_local(n, esz, send, nrows, rowstride, rowidx, sendcounts, sdispls, nullptr, none, none, rowcount);
  if (rc != kRowsOk) return rc;
  // the recv side: blocks of records against each other, the matrix and the list (a "matrix" whose
  // element is one byte describes the same address ranges: extent and stride in bytes)
  bool any_s = false;
  for (int q = 0; q < n; ++q) any_s = any_s || sendcounts[q] != 0;
  const uint64_t top = ~(uint64_t)0;
  rc = rows_check_local(n, 1, nullptr, 0, (size_t)P, nullptr, none, none, recv, recvcounts, rdispls, (size_t)P);
  if (rc != kRowsOk || !any_s) return rc;
  const uint64_t ext = rows_extent_bytes(nrows, rowstride, rowcount, esz);
  const uint64_t sbase = (uint64_t)(uintptr_t)send, ibase = (uint64_t)(uintptr_t)rowidx, rbase = (uint64_t)(uintptr_t)recv;
  uint64_t ilo = top, ihi = 0;
  for (int q = 0; q < n; ++q) {
    if (sendcounts[q] == 0) continue;
    ilo = sdispls[q] * 4 < ilo ? sdispls[q] * 4 : ilo;
    ihi = (sdispls[q] + sendcounts[q]) * 4 > ihi ? (sdispls[q] + sendcounts[q]) * 4 : ihi;
  }
  for (int q = 0; q < n; ++q) {
    if (recvcounts[q] == 0) continue;
    const uint64_t b = rbase + rdispls[q] * P, l = recvcounts[q] * P;
    if (ext && var_ranges_overlap(b, l, sbase, ext)) return kRowsSendRecvOverlap;
    if (var_ranges_overlap(b, l, ibase + ilo, ihi - ilo)) return kRowsSendRecvOverlap;
  }
  return kRowsOk;
}

// ---------------------------------------------------------------- the kernels' view
// The per-destination blocks of this rank (rowsmx_push's second by-value argument; rowsmx_pack takes
// the same with dst the local addresses; rowsmx4_push and rowsmx4_pack alike).  Indexed by destination rank q.
struct MxArgs {
  const char* src;        // the matrix (rowsmx_pack; rowsmx_push reads p.send)
  const int32_t* rowidx;  // device-readable; read when the kernel runs
  uint64_t stride_bytes;  // rowstride * 2
  uint32_t rowcount;      // elements per row
  uint32_t nrows;         // indices outside [0, nrows) give records of zero bytes
  uint64_t idx_off[16];   // sdispls[q]
  char* dst[16];          // where the block's first record goes (rank q's recv + its rdispls[rank] * P)
  uint64_t count[16];     // records (0: nothing goes to q)
  int32_t n;
  int32_t f16;            // the elements are fp16 (else bf16)
};

// How a wave shares its lanes among rows: a lane quantises 16 consecutive elements, so a block of 32
// is a lane pair.  Rows of 1024 elements and more take the wave whole, one pass per 1024 elements;
// narrower rows share a pass, rowcount / 16 lanes per row and 1024 / rowcount rows at once.
//
// `rows` must be a power of two (so it divides 64): the walk (kernels.hip mx_walk) holds the indices of
// 64 records, advances by `rows` records a pass and picks a record's index out of that batch alone, so
// a pass must never straddle two batches.  Lanes at and beyond lanes * rows are idle.
struct MxLanes {
  uint32_t lanes;   // lanes per row (MXFP8: a multiple of 8, MXFP4: of 4; at most 64)
  uint32_t rows;    // rows per pass: a power of two, rows * lanes <= 64
  uint32_t passes;  // passes per row
};
MNCCL_HD MxLanes mx_lanes(uint32_t rowcount) {
  MxLanes g;
  g.lanes = rowcount >= kMxPassElems ? 64u : rowcount / 16u;
  g.rows = 64u / g.lanes;
  g.passes = (rowcount + kMxPassElems - 1) / kMxPassElems;
  return g;
}

// The same for MXFP4: a lane quantises a whole block of 32 consecutive elements into one 16-byte
// vector of nibbles.  Rows of 2048 elements and more take the wave whole, one pass per 2048 elements;
// narrower rows share a pass, rowcount / 32 lanes per row and the largest power of two of rows that
// fits 64 lanes at once (1152 elements: 36 lanes, one row, 28 lanes idle; 384 elements: 12 lanes,
// 4 rows and not 5, 16 lanes idle; 640 elements: 20 lanes, 2 rows and not 3, 24 lanes idle).  Unlike
// MXFP8's lane counts (8, 16, 32, 64), these do not all divide 64: see MxLanes for why rows must.
MNCCL_HD MxLanes mx4_lanes(uint32_t rowcount) {
  MxLanes g;
  g.lanes = rowcount >= kMx4PassElems ? 64u : rowcount / kMxBlock;
  g.rows = 1u << (31 - __builtin_clz(64u / g.lanes));  // (lanes >= 4 for every legal rowcount; 64 / lanes >= 1)
  g.passes = (rowcount + kMx4PassElems - 1) / kMx4PassElems;
  return g;
}

// ---------------------------------------------------------------- the host quantiser (the simulator's)
inline float mx_widen(uint16_t x, bool f16) {
  uint32_t u;
  if (!f16) {
    u = (uint32_t)x << 16;
  } else {
    const uint32_t s = (uint32_t)(x & 0x8000u) << 16, e = (x >> 10) & 31u, m = x & 0x3ffu;
    if (e == 31) u = s | 0x7f800000u | (m << 13);
    else if (e) u = s | ((e + 112u) << 23) | (m << 13);
    else {
      const float v = ldexpf((float)m, -24);  // exact: m < 2^10
      memcpy(&u, &v, 4);
      u |= s;
    }
  }
  float f;
  memcpy(&f, &u, 4);
  return f;
}

// a finite float onto e4m3's grid: nearest even, subnormals included, saturated to +-448
inline uint8_t mx_encode_e4m3(float v) {
  uint32_t u;
  memcpy(&u, &v, 4);
  const uint8_t sign = (uint8_t)((u >> 24) & 0x80u);
  const float a = fabsf(v);
  if (a >= 448.0f) return sign | 0x7e;
  if (a < 0.015625f) return sign | (uint8_t)nearbyintf(a * 512.0f);  // steps of 2^-9; 8 is the smallest normal
  uint32_t e = ((u >> 23) & 0xffu) - 120u, m = (u >> 20) & 7u;        // e4m3's biased exponent, 1 .. 15
  const uint32_t rem = u & 0xfffffu;
  uint32_t b = (e << 3) | m;
  if (rem > 0x80000u || (rem == 0x80000u && (m & 1u))) ++b;
  return sign | (uint8_t)(b > 0x7eu ? 0x7eu : b);
}

// one row of `rowcount` bf16 / fp16 elements into its record
inline void mx_quantise_row(const uint16_t* row, bool f16, uint32_t rowcount, uint8_t* rec) {
  for (uint32_t b = 0; b < rowcount / kMxBlock; ++b) {
    float x[kMxBlock];
    uint32_t amax = 0;
    for (uint32_t i = 0; i < kMxBlock; ++i) {
      x[i] = mx_widen(row[b * kMxBlock + i], f16);
      uint32_t u;
      memcpy(&u, &x[i], 4);
      u &= 0x7fffffffu;
      amax = u > amax ? u : amax;
    }
    const uint32_t s = mx_scale_byte(amax >> 23);
    rec[rowcount + b] = (uint8_t)s;
    for (uint32_t i = 0; i < kMxBlock; ++i)
      rec[b * kMxBlock + i] = s == 255u ? 0x7f : mx_encode_e4m3(ldexpf(x[i], 127 - (int)s));
  }
}

// a finite float onto e2m1's grid {0, 0.5, 1, 1.5, 2, 3, 4, 6}: nearest, ties to the even code, saturated to +-6
inline uint8_t mx4_encode_e2m1(float v) {
  uint32_t u;
  memcpy(&u, &v, 4);
  const float a = fabsf(v);
  return (uint8_t)(((u >> 28) & 8u) | (uint32_t)((a > 0.25f) + (a >= 0.75f) + (a > 1.25f) + (a >= 1.75f) + (a > 2.5f) +
                                                 (a >= 3.5f) + (a > 5.0f)));
}

// one row of `rowcount` bf16 / fp16 elements into its MXFP4 record
inline void mx4_quantise_row(const uint16_t* row, bool f16, uint32_t rowcount, uint8_t* rec) {
  for (uint32_t b = 0; b < rowcount / kMxBlock; ++b) {
    float x[kMxBlock];
    uint32_t amax = 0;
    for (uint32_t i = 0; i < kMxBlock; ++i) {
      x[i] = mx_widen(row[b * kMxBlock + i], f16);
      uint32_t u;
      memcpy(&u, &x[i], 4);
      u &= 0x7fffffffu;
      amax = u > amax ? u : amax;
    }
    const uint32_t s = mx4_scale_byte(amax >> 23);
    rec[rowcount / 2 + b] = (uint8_t)s;
    for (uint32_t i = 0; i < kMxBlock; i += 2) {
      // (an underflow of the scaling ends below 0.25 either way: code 0)
      const uint8_t lo = mx4_encode_e2m1(ldexpf(x[i], 127 - (int)s)), hi = mx4_encode_e2m1(ldexpf(x[i + 1], 127 - (int)s));
      rec[(b * kMxBlock + i) / 2] = s == 255u ? 0x77 : (uint8_t)(lo | hi << 4);
    }
  }
}

}  // namespace mnccl
