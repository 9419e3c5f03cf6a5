"""ctypes front end of the simulator's entry point for sequences that include ncclAllToAllv
(csrc/sim.cpp mnccl_sim_varblock), of the exported host-side rules (csrc/varblock.h), and the
permutation a variable all-to-all is, computed with numpy slicing.

A call's shape is a Layout: the n x n count matrix C (C[r][q] elements go from rank r to rank q) and
every rank's send / recv displacements.  Buffers are seeded random BYTES, different per rank and
seed; a recv starts as FILL bytes with GUARD more behind it, so the gaps between the blocks and the
guard must come back unchanged.
"""
import ctypes

import numpy as np

import sim_alltoall_api as A

ALLREDUCE, REDUCE_SCATTER, ALLGATHER, BROADCAST, REDUCE, ALLTOALL, ALLTOALLV = range(7)
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
        L.mnccl_sim_varblock.argtypes = [i, i, P(i), P(i), P(u64), P(i), P(vp), P(vp), i, P(u64), P(u64), P(u64), i, u64, u64,
                                         i, i, u64, P(u64)]
        L.mnccl_varblock_check_local.argtypes = [i, i, vp, P(sz), P(sz), vp, P(sz), P(sz)]
        L.mnccl_varblock_matrix_mismatch.argtypes = [i, P(u64), P(u64)]
        L.mnccl_varblock_len.argtypes = [u64, u64, u64]
        L.mnccl_varblock_len.restype = u64
        _ready = True
    return L


def check_local(esz, send, sendcounts, sdispls, recv, recvcounts, rdispls):
    """varblock_check_local on one rank's arguments (addresses as integers, never dereferenced):
    0 ok, 1 NULL buffer, 2 overflow, 3 recv blocks overlap, 4 recv overlaps send."""
    n = len(sendcounts)
    arr = lambda a: (ctypes.c_size_t * n)(*a)
    return load().mnccl_varblock_check_local(n, esz, send, arr(sendcounts), arr(sdispls), recv, arr(recvcounts), arr(rdispls))


def matrix_mismatch(sendcounts, recvcounts):
    """varblock_matrix_mismatch on every rank's rows: 0, or 1 + r * n + q of the first differing pair."""
    n = len(sendcounts)
    flat = lambda m: (ctypes.c_uint64 * (n * n))(*[int(x) for row in m for x in row])
    return load().mnccl_varblock_matrix_mismatch(n, flat(sendcounts), flat(recvcounts))


def displacements(counts, mode):
    """Displacements of one rank's blocks: "contig" (block q right after block q - 1), "reversed"
    (block n - 1 first) or "gaps" (reversed with 3 elements between and before the blocks)."""
    n = len(counts)
    order = range(n) if mode == "contig" else range(n - 1, -1, -1)
    gap = 3 if mode == "gaps" else 0
    d, at = [0] * n, gap
    for q in order:
        d[q] = at
        at += int(counts[q]) + gap
    return d, at  # and the buffer's length in elements


class Layout:
    def __init__(self, C, mode="contig", esz=4):
        self.C = np.array(C, dtype=np.int64)
        self.n, self.esz, self.mode = len(C), esz, mode
        self.sd, self.rd, self.slen, self.rlen = [], [], [], []
        for r in range(self.n):
            d, m = displacements(self.C[r, :], mode)
            self.sd.append(d)
            self.slen.append(max(m, 1) * esz)
            d, m = displacements(self.C[:, r], mode)
            self.rd.append(d)
            self.rlen.append(max(m, 1) * esz)

    def sends(self, seed):
        return [np.random.default_rng([seed, r, self.n]).integers(0, 256, self.slen[r], dtype=np.uint8)
                for r in range(self.n)]

    def expect(self, sends):
        """Rank q's recv: FILL, with the block from every rank r at rd[q][r]."""
        e = self.esz
        out = []
        for q in range(self.n):
            x = np.full(self.rlen[q], FILL, np.uint8)
            for r in range(self.n):
                c = int(self.C[r, q])
                x[self.rd[q][r] * e:(self.rd[q][r] + c) * e] = sends[r][self.sd[r][q] * e:(self.sd[r][q] + c) * e]
            out.append(x)
        return out


def random_matrix(n, seed, values=(0, 1, 3, 300, 16411)):
    return np.random.default_rng([seed, n]).choice(values, size=(n, n))


def run(n, calls, esz=4, op=0, slice_bytes=1024, channels=4, slots=2, seed=0, min_slice=0):
    """calls: a list of (coll, sched, inputs, inplace, root).  For ALLTOALLV, inputs is (layout, sends);
    the call's recv buffers start as FILL with GUARD bytes behind them, and the guard and the send are
    checked here.  The six other collectives as sim_alltoall_api.run.  Returns each call's per-rank
    recv contents (a variable call's as uint8 without the guard); RuntimeError on deadlock."""
    k = len(calls)
    colls = (ctypes.c_int * k)(*[c[0] for c in calls])
    scheds = (ctypes.c_int * k)(*[c[1] for c in calls])
    roots = (ctypes.c_int * k)(*[c[4] for c in calls])
    counts = (ctypes.c_uint64 * k)()
    vc, vs, vr = ((ctypes.c_uint64 * (k * n * n))() for _ in range(3))
    sp = (ctypes.c_void_p * (k * n))()
    rp = (ctypes.c_void_p * (k * n))()
    keep, outs, checks = [], [], []
    for i, (coll, _, inputs, inplace, root) in enumerate(calls):
        if coll == ALLTOALLV:
            lay, given = inputs
            assert lay.n == n and lay.esz == esz
            sends = [np.array(x, dtype=np.uint8) for x in given]
            full = [np.full(lay.rlen[r] + GUARD, FILL, np.uint8) for r in range(n)]
            recvs = [f[:lay.rlen[r]] for r, f in enumerate(full)]
            for r in range(n):
                for q in range(n):
                    j = (i * n + r) * n + q
                    vc[j], vs[j], vr[j] = int(lay.C[r, q]), lay.sd[r][q], lay.rd[r][q]
            checks.append((i, given, sends, full))
        elif coll == ALLTOALL:
            nbytes = inputs[0].size
            counts[i] = nbytes // (4 * n)
            sends = [np.array(x, dtype=np.uint8) for x in inputs]
            full = [np.full(nbytes + GUARD, FILL, np.uint8) for _ in range(n)]
            recvs = [f[:nbytes] for f in full]
            checks.append((i, inputs, sends, full))
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
            else:
                sends, recvs = xs, [np.full(c, np.nan, np.float32) for _ in range(n)]
        keep.append((sends, recvs))
        for r in range(n):
            sp[i * n + r] = None if sends[r] is None else sends[r].ctypes.data
            rp[i * n + r] = recvs[r].ctypes.data
        outs.append(recvs)
    steps = ctypes.c_uint64()
    rc = load().mnccl_sim_varblock(n, k, colls, scheds, counts, roots, sp, rp, esz, vc, vs, vr, op, slice_bytes, min_slice,
                                   channels, slots, seed, ctypes.byref(steps))
    if rc == -1:
        raise RuntimeError("simulated protocol deadlocked")
    if rc != 0:
        raise ValueError(f"bad simulator arguments (rc={rc})")
    for i, given, sends, full in checks:
        for r in range(n):
            assert np.array_equal(sends[r], given[r]), f"call {i}: rank {r}'s send was written"
            assert np.all(full[r][-GUARD:] == FILL), f"call {i}: rank {r}'s guard bytes were written"
    return outs
