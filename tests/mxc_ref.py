"""mncclAllToAllvCombineMxfp8's decode in numpy (the fold is combine_workers.Shape.expect's); canon(): NaN compares as NaN."""
import numpy as np

import fp8_ref

SCALES = (0, 1, 119, 127, 246, 247, 254, 255)  # subnormal and smallest-normal 2^(s - 127), the dispatch's range, overflow, NaN
_ELEM = {"f32": (np.uint32, np.float32, 0x7FC00000), "f16": (np.uint16, np.float16, 0x7E00), "bf16": (np.uint16, None, 0x7FC0)}


def decode(recs, rowcount):
    """(R, rowcount + rowcount // 32) uint8 records -> (R, rowcount) float32."""
    recs = np.asarray(recs, np.uint8).reshape(-1, rowcount + rowcount // 32)
    s = np.repeat(recs[:, rowcount:].astype(np.int64), 32, axis=1)
    with np.errstate(all="ignore"):
        x = np.ldexp(fp8_ref.decode(recs[:, :rowcount], "e4m3").astype(np.float64), s - 127).astype(np.float32)
    return np.where(s == 255, np.float32(np.nan), x)


def canon(b, dt):
    """A flat uint8 buffer of whole elements (a tail is left alone), in place: every NaN element becomes one quiet NaN."""
    u, f, q = _ELEM[dt]
    e = b[:b.size // np.dtype(u).itemsize * np.dtype(u).itemsize].view(u)
    e[np.isnan((e.astype(np.uint32) << 16).view(np.float32) if f is None else e.view(f))] = q
    return b
