"""ctypes front end of the simulator's entry point for sequences that include mncclAllGatherv and
mncclReduceScatterv (csrc/sim.cpp mnccl_sim_vhalves), of the exported host-side rules (csrc/vhalves.h,
schedule.h vhalf_len), and the two calls' expected results.

A call's shape is a Shape: the n counts, the n displacements (both in elements, the same on every
rank) and the array-side buffer's length.  The gather moves seeded random BYTES and is expected to be
the permutation itself; the fold is fp32 and is expected to be oracle_api.ring_fold on block c laid
into chunk c of an n x max(counts) buffer.  An array-side recv starts as FILL bytes with GUARD more
behind it, a one-block recv sits between two guards: gaps and guards must come back unchanged.
"""
import ctypes

import numpy as np

import sim_alltoall_api as A

ALLREDUCE, REDUCE_SCATTER, ALLGATHER, BROADCAST, REDUCE, ALLTOALL = range(6)
ALLGATHERV, REDUCESCATTERV = 9, 10
RING, READ = A.RING, A.READ
GUARD = A.GUARD
FILL = 0xA5

_ready = False


def load():
    global _ready
    L = A.load()
    if not _ready:
        vp, u64, i, sz = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_size_t
        P = ctypes.POINTER
        L.mnccl_sim_vhalves.argtypes = [i, i, P(i), P(i), P(u64), P(i), P(vp), P(vp), i, P(u64), P(u64), i, u64, u64, i, i,
                                        u64, P(u64)]
        L.mnccl_vhalf_check_local.argtypes = [i, i, i, vp, P(sz), P(sz), vp, sz]
        L.mnccl_vhalf_rows_differ.argtypes = [i, P(u64), P(u64)]
        L.mnccl_vhalf_len.argtypes = [u64, u64, u64]
        L.mnccl_vhalf_len.restype = u64
        L.mnccl_vhalf_vec.argtypes = [i, u64, u64]
        _ready = True
    return L


def check_local(rank, esz, array_buf, counts, displs, one_buf, one_count):
    """vhalf_check_local on one rank's arguments (addresses as integers, never dereferenced): 0 ok,
    1 scalar count != counts[rank], 2 NULL buffer, 3 overflow, 4 blocks overlap, 5 the one-block buffer
    overlaps a block and is not in place."""
    n = len(counts)
    arr = lambda a: (ctypes.c_size_t * n)(*a)
    return load().mnccl_vhalf_check_local(n, rank, esz, array_buf, arr(counts), arr(displs), one_buf, one_count)


def rows_differ(counts, displs):
    """vhalf_rows_differ on every rank's arrays (n x n): 0, or 1 + r * n + q of the first entry that
    differs from rank 0's."""
    n = len(counts)
    flat = lambda m: (ctypes.c_uint64 * (n * n))(*[int(x) for row in m for x in row])
    return load().mnccl_vhalf_rows_differ(n, flat(counts), flat(displs))


class Shape:
    """counts with displacements "contig" (block q right after block q - 1), "reversed" (block n - 1
    first) or "gaps" (reversed, with 3 elements before and between the blocks)."""

    def __init__(self, counts, mode="contig"):
        self.counts = [int(c) for c in counts]
        self.n, self.mode = len(self.counts), mode
        order = range(self.n) if mode == "contig" else range(self.n - 1, -1, -1)
        gap = 3 if mode == "gaps" else 0
        self.displs, at = [0] * self.n, gap
        for q in order:
            self.displs[q] = at
            at += self.counts[q] + gap
        self.length = max(at, 1)  # the array-side buffer, in elements
        self.M = max(self.counts)

    def blocks(self, seed, esz):
        """Rank r's send of the gather: counts[r] * esz seeded random bytes."""
        return [np.random.default_rng([seed, r, self.n, 11]).integers(0, 256, self.counts[r] * esz, dtype=np.uint8)
                for r in range(self.n)]

    def gather_expect(self, blocks, esz):
        """Every rank's recv: FILL, with rank q's block at displs[q]."""
        x = np.full(self.length * esz, FILL, np.uint8)
        for q in range(self.n):
            x[self.displs[q] * esz:(self.displs[q] + self.counts[q]) * esz] = blocks[q]
        return x

    def laid_out(self, xs):
        """Every rank's send with block c laid into chunk c of an n x M buffer (the padding zero)."""
        out = []
        for x in xs:
            y = np.zeros(self.n * max(self.M, 1), dtype=x.dtype)
            for c in range(self.n):
                y[c * self.M:c * self.M + self.counts[c]] = x[self.displs[c]:self.displs[c] + self.counts[c]]
            out.append(y)
        return out

    def fold_expect(self, xs, dtype="f32", op="sum", fold=None):
        """Rank r's recv: oracle_api.ring_fold (or `fold`, same signature) on block c laid into chunk c."""
        import oracle_api as O
        full = (fold or O.ring_fold)(self.laid_out(xs), dtype, op)
        return [full[r * self.M:r * self.M + self.counts[r]] for r in range(self.n)]


def _guarded(nbytes):
    full = np.full(nbytes + 2 * GUARD, FILL, np.uint8)
    return full, full[GUARD:GUARD + nbytes]


def run(n, calls, esz=4, op=0, slice_bytes=1024, channels=4, slots=2, seed=0, min_slice=0):
    """calls: a list of (coll, sched, inputs, inplace, root).

    ALLGATHERV: inputs is (shape, blocks), blocks[r] rank r's counts[r] * esz bytes; a rank with an
    empty block passes NULL for its send.  In place: the send is the block's place in the recv.  The
    call's entry in the result is every rank's recv as uint8 (without the guard).
    REDUCESCATTERV: inputs is (shape, xs), xs[r] rank r's send of shape.length fp32 elements; a rank with
    an empty block passes NULL for its recv.  In place: the recv is block r of the send.  The call's
    entry is every rank's recv as float32 (counts[r] elements).
    The six collectives 0 .. 5 as sim_alltoall_api.run.
    Checked here after the run: the guards, and the sends of every call that is not in place.
    Raises RuntimeError on deadlock."""
    k = len(calls)
    colls = (ctypes.c_int * k)(*[c[0] for c in calls])
    scheds = (ctypes.c_int * k)(*[c[1] for c in calls])
    roots = (ctypes.c_int * k)(*[c[4] for c in calls])
    counts = (ctypes.c_uint64 * k)()
    vc, vd = ((ctypes.c_uint64 * (k * n))() for _ in range(2))
    sp = (ctypes.c_void_p * (k * n))()
    rp = (ctypes.c_void_p * (k * n))()
    keep, outs, guards, untouched = [], [], [], []
    for i, (coll, _, inputs, inplace, root) in enumerate(calls):
        if coll in (ALLGATHERV, REDUCESCATTERV):
            sh, given = inputs
            assert sh.n == n
            for q in range(n):
                vc[i * n + q], vd[i * n + q] = sh.counts[q], sh.displs[q]
            sends, recvs = [], []
            for r in range(n):
                c, d = sh.counts[r], sh.displs[r]
                if coll == ALLGATHERV:
                    full = np.full(sh.length * esz + GUARD, FILL, np.uint8)
                    guards.append((i, full[-GUARD:]))
                    recv = full[:sh.length * esz]
                    if c == 0:
                        send = None
                    elif inplace:
                        send = recv[d * esz:(d + c) * esz]
                        send[:] = given[r]
                    else:
                        send = np.array(given[r], dtype=np.uint8)
                        untouched.append((i, send, given[r], f"rank {r}'s send"))
                else:
                    send = np.array(given[r], dtype=np.float32)
                    if c == 0:
                        recv = None
                    elif inplace:
                        recv = send[d:d + c]
                    else:
                        full, view = _guarded(4 * c)
                        guards.append((i, full[:GUARD]))
                        guards.append((i, full[-GUARD:]))
                        recv = view.view(np.float32)
                    if not inplace:
                        untouched.append((i, send, given[r], f"rank {r}'s send"))
                sends.append(send)
                recvs.append(recv)
            ret = recvs if coll == ALLGATHERV else [np.zeros(0, np.float32) if x is None else x for x in recvs]
            if coll == REDUCESCATTERV and inplace:
                # everything of an in-place send outside the own block stays what it was
                for r in range(n):
                    mask = np.ones(sh.length, bool)
                    mask[sh.displs[r]:sh.displs[r] + sh.counts[r]] = False
                    untouched.append((i, sends[r].view(np.uint32)[mask], np.array(given[r], np.float32).view(np.uint32)[mask],
                                      f"rank {r}'s send outside its own block"))
        elif coll == ALLTOALL:
            nbytes = inputs[0].size
            counts[i] = nbytes // (4 * n)
            sends = [np.array(x, dtype=np.uint8) for x in inputs]
            recvs = [np.full(nbytes, FILL, np.uint8) for _ in range(n)]
            ret = recvs
        else:
            xs = [np.array(x, dtype=np.float32) for x in inputs]
            c = xs[0].size
            counts[i] = c
            if coll == ALLREDUCE:
                sends, recvs = xs, (xs if inplace else [np.full_like(x, np.nan) for x in xs])
            elif coll == REDUCE_SCATTER:
                counts[i] = c // n
                sends, recvs = xs, [np.full(c // n, np.nan, np.float32) for _ in range(n)]
            elif coll == ALLGATHER:
                sends, recvs = xs, [np.full(n * c, np.nan, np.float32) for _ in range(n)]
            elif coll == BROADCAST:
                sends = [xs[r] if r == root else None for r in range(n)]
                recvs = [np.full(c, np.nan, np.float32) for _ in range(n)]
            elif coll == REDUCE:
                sends, recvs = xs, [np.full(c, np.nan, np.float32) for _ in range(n)]
            else:
                raise ValueError(f"collective {coll} is not one this front end runs")
            ret = recvs
        keep.append((sends, recvs))
        for r in range(n):
            sp[i * n + r] = None if sends[r] is None else sends[r].ctypes.data
            rp[i * n + r] = None if recvs[r] is None else recvs[r].ctypes.data
        outs.append(ret)
    steps = ctypes.c_uint64()
    rc = load().mnccl_sim_vhalves(n, k, colls, scheds, counts, roots, sp, rp, esz, vc, vd, op, slice_bytes, min_slice,
                                  channels, slots, seed, ctypes.byref(steps))
    if rc == -1:
        raise RuntimeError("simulated protocol deadlocked")
    if rc != 0:
        raise ValueError(f"bad simulator arguments (rc={rc})")
    for i, g in guards:
        assert np.all(g == FILL), f"call {i}: guard bytes were written"
    for i, buf, was, what in untouched:
        assert np.array_equal(buf, was), f"call {i}: {what} was written"
    return outs
