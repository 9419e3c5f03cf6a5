"""What mncclAllToAllvRowsMxfp8 delivers for a row (include/mini_nccl_ext.h has the rule), from numpy alone: per block of
32, E = the largest f32 exponent field; 255: scale 0xFF, bytes 0x7F; else s = max(E - 8, 0), fp8_ref.encode(x * 2^(127 - s))."""
import numpy as np

import fp8_ref

SPECIALS = {False: (0x0000, 0x3F80, 0x43E0, 0x7F7F, 0x0001, 0x0080),  # bf16: 0, 1, 448, largest, smallest, 2^-126
            True: (0x0000, 0x3C00, 0x5F00, 0x7BFF, 0x0001, 0x0000)}   # fp16 (2^-126 is 0 there)


def quantise(rows, f16):
    """(R, rowcount) uint16 patterns -> (R, rowcount + rowcount // 32) uint8 records."""
    rows = np.ascontiguousarray(rows, np.uint16)
    f = rows.view(np.float16).astype(np.float32) if f16 else (rows.astype(np.uint32) << 16).view(np.float32)
    f = f.reshape(rows.shape[0], -1, 32)
    E = ((f.view(np.uint32) & 0x7FFFFFFF).max(-1) >> 23).astype(np.int64)
    s = np.where(E == 255, 255, np.maximum(E - 8, 0))
    with np.errstate(all="ignore"):
        y = np.ldexp(f.astype(np.float64), (127 - s)[..., None]).astype(np.float32)
    codes = np.where((s == 255)[..., None], 0x7F, fp8_ref.encode(y, "e4m3"))
    return np.concatenate([codes.reshape(rows.shape[0], -1), s], axis=1).astype(np.uint8)


def sweep(f16):
    """All 65 536 patterns in blocks of 32, then again with element 31 of every block replaced by each special."""
    base = np.arange(65536, dtype=np.uint16)
    out = [base]
    for v in SPECIALS[f16]:
        out.append(base.copy())
        out[-1][31::32] = v
    return np.concatenate(out)
