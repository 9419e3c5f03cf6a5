"""What mncclAllToAllvRowsMxfp4 delivers for a row (include/mini_nccl_ext.h has the rule), from numpy alone: float64
ldexp, the rule's seven comparisons, element 2i in the low nibble of byte i, then the scale bytes."""
import numpy as np

SPECIALS = {False: (0x0000, 0x3F80, 0x40C0, 0x7F7F, 0x0001, 0x0080),  # bf16: 0, 1, 6, largest, smallest, 2^-126
            True: (0x0000, 0x3C00, 0x4600, 0x7BFF, 0x0001, 0x0000)}   # fp16 (2^-126 is 0 there)


def quantise(rows, f16):
    """(R, rowcount) uint16 patterns -> (R, rowcount // 2 + rowcount // 32) uint8 records."""
    rows = np.ascontiguousarray(rows, np.uint16)
    f = rows.view(np.float16).astype(np.float32) if f16 else (rows.astype(np.uint32) << 16).view(np.float32)
    f = f.reshape(rows.shape[0], -1, 32)
    E = ((f.view(np.uint32) & 0x7FFFFFFF).max(-1) >> 23).astype(np.int64)
    s = np.where(E == 255, 255, np.maximum(E - 2, 0))
    with np.errstate(all="ignore"):
        a = np.abs(np.ldexp(f.astype(np.float64), (127 - s)[..., None]))
        mag = sum(((a > 0.25), (a >= 0.75), (a > 1.25), (a >= 1.75), (a > 2.5), (a >= 3.5), (a > 5.0))).astype(np.uint8)
    codes = np.where((s == 255)[..., None], 7, mag | (f.view(np.uint32) >> 28 & 8)).astype(np.uint8).reshape(rows.shape[0], -1)
    return np.concatenate([codes[:, 0::2] | codes[:, 1::2] << 4, s.astype(np.uint8)], axis=1)


def sweep(f16):
    """All 65 536 patterns in blocks of 32, then again with element 31 of every block replaced by each special."""
    out = np.tile(np.arange(65536, dtype=np.uint16), (7, 1))
    out[1:, 31::32] = np.array(SPECIALS[f16], np.uint16)[:, None]
    return out.reshape(-1)
