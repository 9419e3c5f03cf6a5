// rowblock.h -- the host-side rules of mncclAllToAllvRows (ncclAllToAllv whose send blocks are
// gathered by a device-side list of row indices), as pure functions: no HIP, no communicator.
// Comm::all_to_all_v_rows applies them, the rendezvous carries the rows (varblock.h VarRow, with
// kVarRows in `flags` and the row length in `pad`), kernels.hip (rows_push, rows_pack) and the
// simulator library share the slice rule below, and the simulator exports all of it so the CPU suite
// can call it on hand-made cases.
//
// The send side is a matrix of `nrows` rows, row t at element t * rowstride, of which the first
// `rowcount` elements travel.  The block for rank q is the rows rowidx[sdispls[q] + i], i <
// sendcounts[q], in that order; it lands packed, rows of rowcount elements with no stride, at row
// rdispls[r] of rank q's recv.  Counts and displacements are in ROWS on both sides.  An index outside
// [0, nrows) stands for a row of zero bytes.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "schedule.h"
#include "varblock.h"

namespace mnccl {

// The local checks' verdicts, in the order they are made
enum RowsLocal : int {
  kRowsOk = 0,
  kRowsZeroRow = 1,          // rowcount == 0 with a non-zero count
  kRowsStride = 2,           // rowstride < rowcount
  kRowsTooManyRows = 3,      // nrows > INT32_MAX: no int32 index could name the last rows
  kRowsNullBuffer = 4,       // a NULL sendbuff / rowidx / recvbuff with a non-zero count on that side
  kRowsOverflow = 5,         // a size or an address overflows size_t (a row of 2 GiB or more counts as that)
  kRowsRecvOverlap = 6,      // two non-empty recv blocks overlap
  kRowsSendRecvOverlap = 7   // a non-empty recv block overlaps the send matrix or the used part of rowidx
};

// bytes from the matrix's first to past its last travelling element (0: no rows); no overflow: checked before
inline uint64_t rows_extent_bytes(uint64_t nrows, uint64_t rowstride, uint64_t rowcount, int esz) {
  return nrows == 0 ? 0 : ((nrows - 1) * rowstride + rowcount) * (uint64_t)esz;
}

// One rank's arguments.  esz: the element size in bytes; the arrays hold n entries.
inline int rows_check_local(int n, int esz, const void* send, size_t nrows, size_t rowstride, const int32_t* rowidx,
                            const size_t* sendcounts, const size_t* sdispls, const void* recv, const size_t* recvcounts,
                            const size_t* rdispls, size_t rowcount) {
  bool any_s = false, any_r = false;
  for (int q = 0; q < n; ++q) {
    any_s = any_s || sendcounts[q] != 0;
    any_r = any_r || recvcounts[q] != 0;
  }
  if (rowcount == 0 && (any_s || any_r)) return kRowsZeroRow;
  if (rowstride < rowcount) return kRowsStride;
  if (nrows > (size_t)INT32_MAX) return kRowsTooManyRows;
  if ((any_s && (!send || !rowidx)) || (any_r && !recv)) return kRowsNullBuffer;
  const uint64_t e = (uint64_t)esz, top = ~(uint64_t)0;
  if (rowcount > (uint64_t)INT32_MAX / e) return kRowsOverflow;
  if (!any_s && !any_r) return kRowsOk;  // an idle rank: its buffers are not used
  const uint64_t rb = rowcount * e;
  // the recv side is ncclAllToAllv's with rows for elements
  const size_t none[kVarMaxRanks] = {};
  const int rv = varblock_check_local(n, (int)rb, nullptr, none, none, recv, recvcounts, rdispls);
  if (rv == kVarOverflow) return kRowsOverflow;
  if (rv == kVarRecvOverlap) return kRowsRecvOverlap;
  if (!any_s) return kRowsOk;
  // the send matrix and the used entries of rowidx, as address ranges
  if (rowstride > top / e || (nrows > 1 && (nrows - 1) > (top - rb) / (rowstride * e))) return kRowsOverflow;
  const uint64_t ext = rows_extent_bytes(nrows, rowstride, rowcount, esz), sbase = (uint64_t)(uintptr_t)send;
  if (sbase > top - ext) return kRowsOverflow;
  const uint64_t ibase = (uint64_t)(uintptr_t)rowidx;
  uint64_t ilo = top, ihi = 0;
  for (int q = 0; q < n; ++q) {
    const uint64_t c = sendcounts[q], d = sdispls[q];
    if (c == 0) continue;
    if (d > top - c || d + c > top / 4 || ibase > top - (d + c) * 4) return kRowsOverflow;
    ilo = d * 4 < ilo ? d * 4 : ilo;
    ihi = (d + c) * 4 > ihi ? (d + c) * 4 : ihi;
  }
  const uint64_t rbase = (uint64_t)(uintptr_t)recv;
  for (int q = 0; q < n; ++q) {
    if (recvcounts[q] == 0) continue;
    const uint64_t b = rbase + rdispls[q] * rb, l = recvcounts[q] * rb;
    if (ext && var_ranges_overlap(b, l, sbase, ext)) return kRowsSendRecvOverlap;
    if (var_ranges_overlap(b, l, ibase + ilo, ihi - ilo)) return kRowsSendRecvOverlap;
  }
  return kRowsOk;
}

// ---------------------------------------------------------------- the kernels' view
// The per-destination blocks of this rank (a second by-value kernel argument of rows_push, as
// VarBlockArgs is varblock_push's).  Indexed by destination rank q; this rank's own block at [rank].
struct RowsArgs {
  const int32_t* rowidx;   // device-readable; read when the kernel runs
  uint64_t stride_bytes;   // rowstride * element size
  uint32_t row_bytes;      // rowcount * element size (< 2 GiB)
  uint32_t nrows;          // indices outside [0, nrows) give rows of zero bytes
  uint64_t idx_off[16];    // sdispls[q]: the block's first entry of rowidx
  uint64_t dst_off[16];    // byte offset of the block in rank q's recv (rank q's rdispls[rank] * row_bytes)
  uint64_t bytes[16];      // sendcounts[q] * row_bytes (0: nothing goes to q)
  uint32_t vec_mask;       // bit q: the 16-byte path (rows_vec_ok)
  uint32_t pad;
};

// A destination takes the 16-byte path when every row's source and destination are dword-aligned
inline bool rows_vec_ok(const void* send, uint64_t stride_bytes, uint64_t row_bytes, uint64_t dst_addr) {
  return ((uint64_t)(uintptr_t)send | stride_bytes | row_bytes | dst_addr) % 4 == 0;
}

// recv_of[q]: this rank's address of rank q's recv; peer_rdispl[q]: rank q's rdispls[rank], in rows
inline void rows_fill_args(RowsArgs* v, int n, int esz, const void* send, size_t nrows, size_t rowstride,
                           const int32_t* rowidx, const size_t* sendcounts, const size_t* sdispls, size_t rowcount,
                           const void* const* recv_of, const uint64_t* peer_rdispl) {
  *v = RowsArgs{};
  v->rowidx = rowidx;
  v->stride_bytes = (uint64_t)rowstride * (uint64_t)esz;
  v->row_bytes = (uint32_t)(rowcount * (size_t)esz);
  v->nrows = (uint32_t)nrows;
  for (int q = 0; q < n; ++q) {
    v->idx_off[q] = sdispls[q];
    v->dst_off[q] = peer_rdispl[q] * (uint64_t)v->row_bytes;
    v->bytes[q] = (uint64_t)sendcounts[q] * (uint64_t)v->row_bytes;
    if (v->bytes[q] && rows_vec_ok(send, v->stride_bytes, v->row_bytes, (uint64_t)(uintptr_t)recv_of[q] + v->dst_off[q]))
      v->vec_mask |= 1u << q;
  }
}

// The slice rule.  A block is the virtual packed sequence of its rows; the call's slices are cut for
// the largest block of the matrix (varblock_len_at), so slice [a, b) may begin and end inside a row.
// A row moves as UNITS at fixed places of the row -- whole 16-byte vectors from its start, then
// elements (the last row_bytes % 16 bytes of a vector destination, every byte of the others) -- and a
// unit belongs to the slice that holds its FIRST byte: a vector that straddles a cut travels whole
// with the earlier slice, so every byte of the block is stored exactly once whatever the row length,
// and no access ever leaves its row.  Of row j's units at row offsets lo + i * u, i < cnt, the ones
// of slice [a, b) are [*i0, *i1).  row_start = j * row_bytes; the row has a byte in the slice.
MNCCL_HD void rows_units(uint64_t a, uint64_t b, uint64_t row_start, uint32_t lo, uint32_t u, uint32_t cnt,
                         uint32_t* i0, uint32_t* i1) {
  const uint64_t s = row_start + lo;
  const uint64_t f = a > s ? (a - s + u - 1) / u : 0, l = b > s ? (b - s + u - 1) / u : 0;
  *i0 = f < cnt ? (uint32_t)f : cnt;
  *i1 = l < cnt ? (uint32_t)l : cnt;
}

// Rows at least this many 16-byte vectors long are walked one row at a time by the whole wave;
// shorter ones share a pass, lane l serving row l / units, unit l % units (DESIGN.md "Schedules")
constexpr uint32_t kRowsWideVectors = 64;

}  // namespace mnccl
