"""What a pre-multiplied sum (ncclRedOpCreatePreMulSum) must produce, from numpy and the oracle
alone, and the inputs the GPU tests run on (tests/test_premul_gpu.py, tests/test_premul_cpu.py).

With s the scalar, every rank's input element becomes y = round_T(s * x) -- one correctly rounded
multiplication in T's arithmetic -- and the y are reduced as ncclSum reduces them.  So the expected
values are the oracle's (oracle_api.allreduce / ring_fold, op "sum") on inputs scaled here in numpy:
float32 / float64 / float16 multiplication, bf16_from_f32(bf16_to_f32(x) * s) for bf16, wrapping
arrays for int32.  An all-reduce's unreduced tail (count % n elements) is the rank's RAW input.
"""
from fractions import Fraction

import numpy as np

import oracle_api as O
import rooted_ref

FLOATS = ("f32", "f64", "f16", "bf16")
DTYPES = ("f32", "f64", "i32", "f16", "bf16")
INT_SCALARS = (3, -7)


def float_scalars(n):
    return (1.0 / n, 0.3, -2.5)


def scalars(dtype, n):
    return INT_SCALARS if dtype == "i32" else float_scalars(n)


def scalar_value(s, dtype):
    """The scalar as ONE value of the datatype (what the op is created with): a numpy scalar of the
    storage type -- for bf16 the 16 bits, rounded to nearest even from float32(s)."""
    if dtype == "bf16":
        return O.bf16_from_f32(np.array([s], np.float32))[0]
    return O.DTYPES[dtype][1](s)


def scalar_arg(s, dtype):
    """scalar_value as mini_nccl.scalar_bytes takes it (bf16: the bits as an int)."""
    v = scalar_value(s, dtype)
    return int(v) if dtype in ("bf16", "i32") else float(v)


def prescale(x, s, dtype):
    """y = round_T(scalar_value(s) * x), element by element, in numpy."""
    sv = scalar_value(s, dtype)
    if dtype == "bf16":
        return O.bf16_from_f32(O.bf16_to_f32(x) * O.bf16_to_f32(np.array([sv], np.uint16))[0])
    if dtype == "i32":
        return ((x.astype(np.int64) * int(sv)) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    with np.errstate(over="ignore", invalid="ignore"):
        return (x * sv).astype(x.dtype)


def allreduce_expect(xs, s, dtype, rank, inplace=False):
    """Rank `rank`'s recv after the all-reduce: the oracle's sum of the scaled inputs, the tail of
    count % n elements from the rank's raw input."""
    n, count = len(xs), xs[0].size
    out = O.allreduce([prescale(x, s, dtype) for x in xs], dtype, "sum", inplace=inplace)[rank]
    body = count // n * n
    out[body:] = xs[rank][body:]
    return out


def reduce_scatter_expect(xs, s, dtype, rank):
    c = xs[0].size // len(xs)
    return O.ring_fold([prescale(x, s, dtype) for x in xs], dtype, "sum")[rank * c:(rank + 1) * c]


def reduce_expect(xs, s, dtype):
    return rooted_ref.reduce_expect([prescale(x, s, dtype) for x in xs], dtype, "sum")


def one_rank_expect(x, s, dtype):
    """nranks == 1: every element scaled, no tail."""
    return prescale(x, s, dtype)


# ---------------------------------------------------------------- exact arithmetic
# (significand bits, smallest normal exponent) of the float formats
FORMAT = {"f16": (11, -14), "bf16": (8, -126), "f32": (24, -126), "f64": (53, -1022)}


def round_fraction(fr, dtype):
    """The exact rational `fr` rounded to nearest even into the format, as a Fraction (no overflow
    handling: the tests' values are far from the formats' ends)."""
    if fr == 0:
        return Fraction(0)
    p, emin = FORMAT[dtype]
    a = abs(fr)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    e = max(e, emin)
    quantum = Fraction(2) ** (e - p + 1)
    q = a / quantum
    k = q.numerator // q.denominator
    rem = q - k
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and k % 2 == 1):
        k += 1
    r = k * quantum
    return -r if fr < 0 else r


def as_fraction(v, dtype):
    """One stored element as an exact rational."""
    if dtype == "bf16":
        return Fraction(float(O.bf16_to_f32(np.array([v], np.uint16))[0]))
    return Fraction(float(v))


def fused_differs(x_first, x_next, s, dtype, limit=4096):
    """Index of the first element at which a contracted multiply-add would be seen, or -1: the
    fold's first step is acc = y_next + y_first with y = round(s * x); fused, it would be
    round(s * x_next + y_first), one rounding of the exact value."""
    sv = as_fraction(scalar_value(s, dtype), dtype)
    y_first, y_next = prescale(x_first, s, dtype), prescale(x_next, s, dtype)
    for i in range(min(limit, x_first.size)):
        acc = as_fraction(y_first[i], dtype)
        two = round_fraction(as_fraction(y_next[i], dtype) + acc, dtype)
        fused = round_fraction(sv * as_fraction(x_next[i], dtype) + acc, dtype)
        if two != fused:
            return i
    return -1


# ---------------------------------------------------------------- the GPU tests' inputs
SEED = 7100


def inputs(n, count, dtype, seed):
    return O.random_inputs(n, count, dtype, seed=seed)


def parity_dtypes(n):
    """All five datatypes at 3 ranks, f32 and bf16 elsewhere, f32 alone past 8 ranks."""
    return DTYPES if n == 3 else ("f32",) if n > 8 else ("f32", "bf16")


# The parity cases of one communicator of n ranks under boundary_cases.ONE (one pipeline): every
# collective x schedule x placement on two shapes per datatype --
#   (a) chunks of 4099 elements and an all-reduce tail of n - 1: the element path for the 2-byte
#       types (odd chunk bytes), vectors and a 12-byte remainder for the 4-byte ones;
#   (b) a last slice of two full batches of the fold's 64 * V vectors, 5 vectors and one element
#       (boundary_cases.fold_batch / chunk_bytes: the kernel's constants, which
#       tests/test_boundary_cases.py holds against the library's own slicing).
# The scalars rotate through the cases so that every (datatype, scalar) pair meets every collective.
RING, READ, AUTO = 0, 2, -1


def shape_b_chunk(n, dtype):
    import boundary_cases as BC
    esz = BC.ESZ[dtype]
    return BC.chunk_bytes(2 * BC.fold_batch(n, esz) + 5, esz) // esz


def parity_cases(n):
    out = []
    for dt in parity_dtypes(n):
        ss = scalars(dt, n)
        for si, (chunk, tail) in enumerate(((4099, n - 1), (shape_b_chunk(n, dt), 0))):
            for ci, coll in enumerate(("ar", "rs", "rd")):
                for ai, algo in enumerate((RING, READ)):
                    for inplace in (False, True):
                        k = len(out)
                        # (the four cases of a collective and schedule take four scalars in a row)
                        out.append(dict(coll=coll, dtype=dt, s=ss[(2 * si + inplace + ci + ai) % len(ss)], chunk=chunk,
                                        tail=tail if coll == "ar" else 0, inplace=inplace, algo=algo,
                                        root=(n - 1) if inplace else 0, seed=SEED + k))
    return out


# Shape (c): the smallest accepted MINI_NCCL_SLICE_SIZE (16 bytes) on 4 pipelines with the default 2
# slots -- a chunk of 100 elements is 25 (f32) or 13 (bf16: the last one 8 bytes, the element path)
# slices, up to 7 iterations per pipeline, so the ring's slots wrap several times.
TINY = {"MINI_NCCL_SLICE_SIZE": "16", "MINI_NCCL_CHANNELS": "4"}


def tiny_slice_cases(n):
    out = []
    for dt in ("f32", "bf16"):
        for coll in ("ar", "rs", "rd"):
            for algo in (RING, READ):
                k = len(out)
                out.append(dict(coll=coll, dtype=dt, s=scalars(dt, n)[k % 3], chunk=100, tail=(n - 1) if coll == "ar" else 0,
                                inplace=k % 2 == 1, algo=algo, root=k % n, seed=SEED + 500 + k))
    return out
