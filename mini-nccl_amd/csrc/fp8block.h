// fp8block.h -- the rules of mncclAllToAllvRowsFp8Block128 (mncclAllToAllvRowsMxfp8 with the "1 x 128"
// activation format of the DeepSeek-V3 recipe: e4m3 elements and one f32 scale per 128 consecutive
// elements of a row), as pure functions: no HIP, no communicator.  The send side, the slice rule, the
// local checks (mx_check_local) and the kernels' argument block (MxArgs) are mxblock.h's; kernels.hip
// (rowsfp8b_push, rowsfp8b_pack) and the simulator share what is below.
//
// Each delivered row is one RECORD of P = rowcount + rowcount / 32 bytes -- MXFP8's size, since
// rowcount / 128 scales of 4 bytes are rowcount / 32 bytes: rowcount e4m3 bytes, then rowcount / 128
// IEEE singles, little-endian, one per block.  Records are whole dwords (rowcount % 128 == 0), so the
// scale part is an aligned float array at row pitch P.
//
// The rule, per block of 128 elements widened exactly to f32: A = the largest magnitude, taken on the
// f32 bit patterns.  A's exponent field 255 (a NaN or an infinity): scale word 0x7FC00000, every element
// 0x7F.  Else a = max(A, 1e-4f), inv = 448.0f / a, scale = a / 448.0f (each one correctly rounded single
// division), the scale word is `scale` and element x becomes encode_e4m3(round_f32(x * inv)): one single
// multiply, one rounding to nearest even onto e4m3's grid, subnormals included, magnitudes of 448 and
// above saturated to +-448, the sign of zero kept.
#pragma once
#include "mxblock.h"

namespace mnccl {

constexpr uint32_t kFp8bBlock = 128;              // elements per scale
constexpr uint32_t kFp8bScaleBytes = 4;           // an IEEE single
constexpr uint32_t kFp8bNanScale = 0x7FC00000u;   // the scale word of a block with a NaN or an infinity
constexpr uint32_t kFp8bFloorBits = 0x38D1B717u;  // 1e-4f: the clamp under the amax
constexpr float kFp8bMax = 448.0f;                // e4m3's largest finite value

// bytes of one record
MNCCL_HD uint64_t fp8b_record_bytes(uint64_t rowcount) { return rowcount + rowcount / kFp8bBlock * kFp8bScaleBytes; }

// the clamped amax of a finite block, as f32 bits (magnitudes order as their bits do)
MNCCL_HD uint32_t fp8b_clamped_amax(uint32_t amax_bits) { return amax_bits > kFp8bFloorBits ? amax_bits : kFp8bFloorBits; }

// ---------------------------------------------------------------- the host quantiser (the simulator's)
// inv and scale of a finite block; volatile: each is one division as written, whatever the flags
inline void fp8b_scales(uint32_t amax_bits, float* inv, float* scale) {
  const uint32_t ab = fp8b_clamped_amax(amax_bits);
  volatile float a, top = kFp8bMax;
  memcpy(const_cast<float*>(&a), &ab, 4);
  volatile float i = top / a, s = a / top;
  *inv = i;
  *scale = s;
}

// one row of `rowcount` bf16 / fp16 elements into its record
inline void fp8b_quantise_row(const uint16_t* row, bool f16, uint32_t rowcount, uint8_t* rec) {
  for (uint32_t b = 0; b < rowcount / kFp8bBlock; ++b) {
    float x[kFp8bBlock];
    uint32_t amax = 0;
    for (uint32_t i = 0; i < kFp8bBlock; ++i) {
      x[i] = mx_widen(row[b * kFp8bBlock + i], f16);
      uint32_t u;
      memcpy(&u, &x[i], 4);
      u &= 0x7fffffffu;
      amax = u > amax ? u : amax;
    }
    uint32_t word = kFp8bNanScale;
    if ((amax >> 23) == 255u) {
      memset(rec + b * kFp8bBlock, 0x7f, kFp8bBlock);
    } else {
      float inv, scale;
      fp8b_scales(amax, &inv, &scale);
      memcpy(&word, &scale, 4);
      for (uint32_t i = 0; i < kFp8bBlock; ++i) {
        volatile float y = x[i];  // (one multiply, rounded to single, before the encoder sees it)
        y = y * inv;
        rec[b * kFp8bBlock + i] = mx_encode_e4m3(y);
      }
    }
    for (uint32_t k = 0; k < 4; ++k) rec[rowcount + 4 * b + k] = (uint8_t)(word >> (8 * k));  // little-endian
  }
}

}  // namespace mnccl
