"""What mncclAllToAllvRowsFp8Block128 delivers for a row (include/mini_nccl_ext.h has the rule), in float32 numpy alone:
per block of 128, A = the largest magnitude; non-finite: scale word 0x7FC00000, bytes 0x7F; else a = max(A, 1e-4),
fp8_ref.encode(x * (448 / a)) and the scale a / 448 as four little-endian bytes behind the row's elements."""
import numpy as np

import fp8_ref

SPECIALS = {False: (0x0000, 0x3F80, 0x43E0, 0x7F7F, 0x0001, 0x38D1),  # bf16: 0, 1, 448, largest, smallest, just under 1e-4
            True: (0x0000, 0x3C00, 0x5F00, 0x7BFF, 0x0001, 0x068D)}   # fp16: the same


def quantise(rows, f16):
    """(R, rowcount) uint16 patterns -> (R, rowcount + rowcount // 32) uint8 records."""
    rows = np.ascontiguousarray(rows, np.uint16)
    f = rows.view(np.float16).astype(np.float32) if f16 else (rows.astype(np.uint32) << 16).view(np.float32)
    f = f.reshape(rows.shape[0], -1, 128)
    A = (f.view(np.uint32) & 0x7FFFFFFF).max(-1).view(np.float32)
    bad = ~np.isfinite(A)
    with np.errstate(all="ignore"):
        a = np.maximum(np.where(bad, np.float32(1), A), np.float32(1e-4))
        inv, scale = np.float32(448) / a, a / np.float32(448)
        y = f * inv[..., None]
    assert inv.dtype == scale.dtype == y.dtype == np.float32
    codes = np.where(bad[..., None], 0x7F, fp8_ref.encode(y, "e4m3")).astype(np.uint8)
    words = np.where(bad, 0x7FC00000, scale.view(np.uint32)).astype("<u4")
    return np.concatenate([codes.reshape(rows.shape[0], -1), words.view(np.uint8).reshape(rows.shape[0], -1)], axis=1)


def sweep(f16):
    """All 65 536 patterns in blocks of 128 (another amax each; NaN / inf blocks, blocks under the clamp), then again with element 127 of every block replaced by each special."""
    out = np.tile(np.arange(65536, dtype=np.uint16), (7, 1))
    out[1:, 127::128] = np.array(SPECIALS[f16], np.uint16)[:, None]
    return out.reshape(-1)
