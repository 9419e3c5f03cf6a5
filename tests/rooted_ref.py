"""What ncclReduce's root holds, built from the oracle as it stands (oracle_api.reduce).

q = ceil(count / n); chunk c is elements [c * q, min((c + 1) * q, count)) -- trailing chunks may be
short or empty, there is no unreduced tail -- and every element of chunk c is folded in the
all-reduce's order for chunk c: acc = x_c, then acc = op(x_k, acc) for k = c + 1, ..., c - 1 (mod n),
the loop oracle_api.ring_fold_parallel runs.  ncclBroadcast's expectation is the root's input.
"""
import numpy as np

import oracle_api as O


def chunk_elems(count, n):
    return (count + n - 1) // n


def reduce_expect(inputs, dtype="f32", op="sum"):
    n = len(inputs)
    _, npd = O.DTYPES[dtype]
    ins = [np.ascontiguousarray(x, dtype=npd) for x in inputs]
    count = ins[0].size
    q = chunk_elems(count, n)
    out = np.empty_like(ins[0])
    for c in range(n):
        lo, hi = min(c * q, count), min((c + 1) * q, count)
        if hi <= lo:
            continue
        acc = ins[c][lo:hi].copy()
        for k in range(1, n):
            acc = O.reduce(ins[(c + k) % n][lo:hi], acc, dtype, op)
        out[lo:hi] = acc
    return out
