"""What the fp8 datatypes (ncclFloat8e4m3 / ncclFloat8e5m2) must produce, from numpy alone: the
reference of tests/test_fp8_cpu.py and tests/test_fp8_gpu.py.  The contract is the one stated in
include/mini_nccl_ext.h ("fp8") and DESIGN.md:

  * both encodings are OCP: e4m3fn (bias 7, no infinities, NaN 0x7f / 0xff, largest finite 448) and
    e5m2 (bias 15, IEEE-like: 0x7c / 0xfc are +-inf, 0x7d..0x7f / 0xfd..0xff NaN, largest finite 57344);
  * Sum, Prod: r = float32(a) op float32(b), one IEEE single-precision operation, then encode(r);
  * Max, Min: (fa > fb) ? a : b and (fa < fb) ? a : b on the decoded values, an operand's byte
    returned unchanged, a the local element and b the incoming one;
  * encode(r): NaN -> a NaN of the type; +-inf -> +-inf (e5m2; e4m3 has none and no fold produces
    one); finite r -> nearest even on the finite grid, subnormals included, SATURATING to the
    largest finite value; the sign of zero is r's;
  * a pre-multiplied sum: y = encode(float32(s) * float32(x)), then the y summed as Sum sums them;
  * association across ranks: chunk c is acc = x_c, then acc = op(x_q, acc) for q = c+1 ... c-1,
    re-encoded after every step.

Everything works on numpy uint8 arrays of codes.  A NaN result may be any NaN code: compare with
mismatches(), which treats two NaNs of the format as equal and nothing else.
"""
import numpy as np

# name -> (ncclDataType_t value, exponent bits, mantissa bits, bias, has infinities)
FORMATS = {"e4m3": (10, 4, 3, 7, False), "e5m2": (11, 5, 2, 15, True)}
OPS = ("sum", "prod", "max", "min")
OP_CODE = {"sum": 0, "prod": 1, "max": 2, "min": 3}


def code(fmt):
    return FORMATS[fmt][0]


def max_code(fmt):
    """The code of the largest finite value (sign bit clear)."""
    _, eb, mb, _, has_inf = FORMATS[fmt]
    top = (1 << eb) - 1
    return ((top - 1) << mb) | ((1 << mb) - 1) if has_inf else (top << mb) | ((1 << mb) - 2)


def decode_table(fmt):
    """float32[256]: the value of every code."""
    _, eb, mb, bias, has_inf = FORMATS[fmt]
    out = np.empty(256, np.float32)
    top = (1 << eb) - 1
    for c in range(256):
        sign = -1.0 if c & 0x80 else 1.0
        e, m = (c >> mb) & top, c & ((1 << mb) - 1)
        if has_inf and e == top:
            v = np.inf if m == 0 else np.nan
        elif not has_inf and e == top and m == (1 << mb) - 1:
            v = np.nan
        elif e == 0:
            v = m * 2.0 ** (1 - bias - mb)
        else:
            v = ((1 << mb) + m) * 2.0 ** (e - bias - mb)
        out[c] = np.float32(sign * v) if v == v else np.float32(np.nan)
    return out


_TABLES = {f: decode_table(f) for f in FORMATS}


def decode(codes, fmt):
    return _TABLES[fmt][np.asarray(codes, np.uint8)]


def max_finite(fmt):
    return float(_TABLES[fmt][max_code(fmt)])


def is_nan(codes, fmt):
    return np.isnan(decode(codes, fmt))


def encode_flags(r, fmt):
    """(codes, saturated): float32 values onto the format by the contract's rule; saturated marks
    the finite values that were clamped to the largest finite value."""
    _, eb, mb, bias, has_inf = FORMATS[fmt]
    r = np.asarray(r, np.float32)
    sign = np.where(np.signbit(r), 0x80, 0).astype(np.int64)
    a = np.abs(r.astype(np.float64))          # exact
    finite = np.isfinite(a)
    af = np.where(finite, a, 0.0)
    _, ex = np.frexp(af)                       # af = m * 2^ex, m in [0.5, 1)
    e = np.maximum(ex - 1, 1 - bias)           # the grid's exponent: at least the smallest normal one
    e = np.where(af == 0, 1 - bias, e)
    e = np.minimum(e, 300)
    step = np.ldexp(1.0, (e - mb).astype(np.int64))
    k = np.rint(af / step).astype(np.int64)    # exact division by a power of two; ties to even
    c = ((e + bias - 1).astype(np.int64) << mb) + k
    mc = max_code(fmt)
    saturated = finite & (c > mc)
    c = np.minimum(c, mc)
    nan_code = 0x7F
    inf_code = (((1 << eb) - 1) << mb) if has_inf else nan_code
    c = np.where(np.isnan(a), nan_code, np.where(np.isinf(a), inf_code, c))
    return (c | sign).astype(np.uint8), saturated


def encode(r, fmt):
    return encode_flags(r, fmt)[0]


def _note(stats, out, saturated, fmt):
    if stats is not None:
        stats["sat"] = stats.get("sat", 0) + int(np.count_nonzero(saturated))
        stats["nan"] = stats.get("nan", 0) + int(np.count_nonzero(is_nan(out, fmt)))


def fold(a, b, fmt, op, stats=None):
    """op(a = local, b = incoming), element by element.  stats (a dict) counts saturated and NaN results."""
    a, b = np.asarray(a, np.uint8), np.asarray(b, np.uint8)
    fa, fb = decode(a, fmt), decode(b, fmt)
    with np.errstate(all="ignore"):
        if op == "sum":
            out, sat = encode_flags(fa + fb, fmt)
        elif op == "prod":
            out, sat = encode_flags(fa * fb, fmt)
        elif op == "max":
            out, sat = np.where(fa > fb, a, b), np.zeros(a.shape, bool)
        elif op == "min":
            out, sat = np.where(fa < fb, a, b), np.zeros(a.shape, bool)
        else:
            raise ValueError(op)
    _note(stats, out, sat, fmt)
    return out


def scale(x, s, fmt, stats=None):
    """y = encode(float32(s) * float32(x)); s is one code."""
    with np.errstate(all="ignore"):
        out, sat = encode_flags(decode(np.uint8(s), fmt) * decode(x, fmt), fmt)
    _note(stats, out, sat, fmt)
    return out


def _enter(xs, s, fmt, stats):
    return [np.asarray(x, np.uint8) if s is None else scale(x, s, fmt, stats) for x in xs]


def _fold_chunk(ys, c, lo, hi, fmt, op, stats):
    n = len(ys)
    acc = ys[c][lo:hi].copy()
    for k in range(1, n):
        acc = fold(ys[(c + k) % n][lo:hi], acc, fmt, "sum" if op == "premul" else op, stats)
    return acc


def ring_fold(xs, fmt, op, s=None, stats=None):
    """The n * (count // n) reduced elements in the library's association (op "premul": scale by the
    code s on the way in, then sum)."""
    n, q = len(xs), xs[0].size // len(xs)
    ys = _enter(xs, s if op == "premul" else None, fmt, stats)
    out = np.empty(n * q, np.uint8)
    for c in range(n):
        out[c * q:(c + 1) * q] = _fold_chunk(ys, c, c * q, (c + 1) * q, fmt, op, stats)
    return out


def allreduce_expect(xs, fmt, op, rank, s=None, stats=None):
    """Rank `rank`'s recv: the fold, then the count % n tail elements of its own raw input."""
    body = ring_fold(xs, fmt, op, s, stats)
    return np.concatenate([body, np.asarray(xs[rank], np.uint8)[body.size:]])


def reduce_scatter_expect(xs, fmt, op, rank, s=None, stats=None):
    q = xs[0].size // len(xs)
    return ring_fold(xs, fmt, op, s, stats)[rank * q:(rank + 1) * q]


def reduce_expect(xs, fmt, op, s=None, stats=None):
    """ncclReduce's root: chunks of ceil(count / n) elements, the trailing ones short or empty, no tail."""
    n, count = len(xs), xs[0].size
    q = (count + n - 1) // n
    ys = _enter(xs, s if op == "premul" else None, fmt, stats)
    out = np.empty(count, np.uint8)
    for c in range(n):
        lo, hi = min(c * q, count), min((c + 1) * q, count)
        if hi > lo:
            out[lo:hi] = _fold_chunk(ys, c, lo, hi, fmt, op, stats)
    return out


def mismatches(got, exp, fmt):
    """(count, first index or -1): bytes that differ, two NaNs of the format counting as equal."""
    got, exp = np.asarray(got, np.uint8), np.asarray(exp, np.uint8)
    bad = (got != exp) & ~(is_nan(got, fmt) & is_nan(exp, fmt))
    idx = np.flatnonzero(bad)
    return int(idx.size), int(idx[0]) if idx.size else -1


# ---------------------------------------------------------------- the GPU tests' inputs
def plain_codes(fmt):
    """Every finite code with |value| < 8 (sums of up to 8 of them and products of up to 3 stay finite
    and below the largest finite value in both formats: nothing saturates, nothing is NaN)."""
    v = _TABLES[fmt]
    return np.flatnonzero(np.isfinite(v) & (np.abs(v) < 8)).astype(np.uint8)


def inputs(n, count, fmt, seed, kind):
    """n arrays of `count` codes: kind "plain" uniform over plain_codes, "wild" uniform over all 256."""
    g = np.random.default_rng(seed)
    if kind == "wild":
        return [g.integers(0, 256, count, dtype=np.uint8) for _ in range(n)]
    pool = plain_codes(fmt)
    return [pool[g.integers(0, pool.size, count)] for _ in range(n)]
