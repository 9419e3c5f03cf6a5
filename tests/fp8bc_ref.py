"""mncclAllToAllvCombineFp8Block128's decode in float32 numpy alone: the e4m3 code's value from a table times its block's single."""
import numpy as np

_c = np.arange(256)
_e, _m = (_c >> 3) & 15, _c & 7
TABLE = np.where(_e == 0, _m * 2.0 ** -9, (8 + _m) * 2.0 ** (_e - 10.0)) * np.where(_c & 0x80, -1.0, 1.0)
TABLE[[0x7F, 0xFF]] = np.nan
TABLE = TABLE.astype(np.float32)  # (exact)
# 1, the dispatch's floor, a subnormal, one that overflows against large codes, a negative, 0, +inf, the dispatch's NaN word
SCALES = np.concatenate([np.array([1.0, np.float32(1e-4) / np.float32(448), 2.0 ** -140, 2.0 ** 120, -0.5, 0.0, np.inf],
                                  np.float32).view(np.uint32), np.array([0x7FC00000], np.uint32)])


def decode(recs, rowcount):  # (R, rowcount + rowcount // 32) uint8 records -> (R, rowcount) float32, one np.float32 multiply each
    recs = np.ascontiguousarray(recs, np.uint8).reshape(-1, rowcount + rowcount // 32)
    s = np.ascontiguousarray(recs[:, rowcount:]).view("<f4").astype(np.float32)
    with np.errstate(all="ignore"):
        x = TABLE[recs[:, :rowcount]] * np.repeat(s, 128, axis=1)
    assert x.dtype == np.float32
    return x
