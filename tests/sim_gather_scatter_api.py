"""ctypes front end of the simulator's entry point for sequences that include ncclGather and
ncclScatter (csrc/sim.cpp mnccl_sim_all_collectives), of their ring tables' per-rank op count
(mnccl_coll_num_ops_at), and the permutations the two are, computed with numpy.

Any of the nine collectives may follow any other, on either schedule, with a root per call, on ONE
simulated communicator state.  A gather's and a scatter's buffers are raw bytes (the simulator only
copies them): seeded random bytes, so NaN payloads and every bit pattern occur.  Every buffer of
the two sits between GUARD bytes that must come back unchanged; a non-root's unused large buffer is
NULL on odd ranks and a buffer of FILL bytes on even ranks that must come back unchanged too.
"""
import ctypes

import numpy as np

import sim_alltoallv_api as V

ALLREDUCE, REDUCE_SCATTER, ALLGATHER, BROADCAST, REDUCE, ALLTOALL, ALLTOALLV, GATHER, SCATTER = range(9)
RING, READ = V.RING, V.READ
GUARD = V.GUARD
FILL = 0xA5

_ready = False


def load():
    global _ready
    L = V.load()
    if not _ready:
        vp, u64, i = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int
        P = ctypes.POINTER
        L.mnccl_sim_all_collectives.argtypes = [i, i, P(i), P(i), P(u64), P(i), P(vp), P(vp), i, P(u64), P(u64), P(u64), i,
                                                u64, u64, i, i, u64, P(u64)]
        L.mnccl_coll_num_ops_at.argtypes = [i, i, i, i]
        _ready = True
    return L


def num_ops_at(coll, n, r, root):
    return load().mnccl_coll_num_ops_at(coll, n, r, root)


def random_bytes(nbytes, *seed):
    return np.random.default_rng(list(seed)).integers(0, 256, nbytes, dtype=np.uint8)


def gather_inputs(n, block_bytes, seed):
    """Rank r's send: one block of seeded random bytes, different per rank and seed."""
    return [random_bytes(block_bytes, seed, r, n, 7) for r in range(n)]


def scatter_input(n, block_bytes, seed):
    """The root's send: n blocks of seeded random bytes."""
    return random_bytes(n * block_bytes, seed, n, 8)


def gather_expect(blocks):
    """The root's recv: rank q's block at q * block_bytes."""
    return np.concatenate(blocks)


def scatter_expect(send, n):
    """Rank q's recv: block q of the root's send."""
    b = send.size // n
    return [send[q * b:(q + 1) * b] for q in range(n)]


def _guarded(nbytes):
    """A buffer of nbytes FILL bytes between two guards: (whole array, the buffer's view)."""
    full = np.full(nbytes + 2 * GUARD, FILL, np.uint8)
    return full, full[GUARD:GUARD + nbytes]


def run(n, calls, op=0, slice_bytes=1024, channels=4, slots=2, seed=0, min_slice=0):
    """calls: a list of (coll, sched, inputs, inplace, root).

    GATHER: inputs[r] is rank r's block as uint8 (a multiple of 4 bytes); `inplace` is the root's
    (its send is block `root` of its recv).  The call's entry in the result is the root's recv.
    SCATTER: inputs is the root's send as uint8 (n blocks); `inplace` is the root's (its recv is block
    `root` of its send).  The call's entry in the result is every rank's recv.
    ALLTOALLV: inputs is (layout, sends) as sim_alltoallv_api.run takes it (4-byte elements).
    The six other collectives as sim_alltoall_api.run.
    Checked here after the run, for every gather and scatter: the guards around every buffer, the
    sends (but an in-place root's), and the FILL buffers the non-roots passed for their unused side.
    Raises RuntimeError on deadlock."""
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
        if coll in (GATHER, SCATTER):
            b = inputs[0].size if coll == GATHER else inputs.size // n
            assert b % 4 == 0 and b > 0
            counts[i] = b // 4
            fulls, sends, recvs, untouched = [], [], [], []
            for r in range(n):
                big_full, big = _guarded(n * b)      # the large buffer: the root's, or a non-root's unused one
                small_full, small = _guarded(b)      # the one-block buffer
                fulls += [big_full, small_full]
                if r == root:
                    if coll == GATHER:
                        small[:] = inputs[r]
                        if inplace:
                            big[r * b:(r + 1) * b] = inputs[r]
                            small = big[r * b:(r + 1) * b]
                    else:
                        big[:] = inputs
                        if inplace:
                            small = big[r * b:(r + 1) * b]
                        else:
                            untouched.append((big, np.array(inputs), f"rank {r}'s send"))
                else:
                    if coll == GATHER:
                        small[:] = inputs[r]
                    if r % 2:
                        big = None
                    else:
                        untouched.append((big, np.full(n * b, FILL, np.uint8), f"rank {r}'s unused buffer"))
                if coll == GATHER:
                    if not (r == root and inplace):
                        untouched.append((small, np.array(inputs[r]), f"rank {r}'s send"))
                    sends.append(small)
                    recvs.append(big)
                else:
                    sends.append(big)
                    recvs.append(small)
            checks.append((i, fulls, untouched))
            ret = recvs[root] if coll == GATHER else recvs
        elif coll == ALLTOALLV:
            lay, given = inputs
            assert lay.n == n and lay.esz == 4
            sends = [np.array(x, dtype=np.uint8) for x in given]
            recvs = [np.full(lay.rlen[r], V.FILL, np.uint8) for r in range(n)]
            for r in range(n):
                for q in range(n):
                    j = (i * n + r) * n + q
                    vc[j], vs[j], vr[j] = int(lay.C[r, q]), lay.sd[r][q], lay.rd[r][q]
            ret = recvs
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
            else:
                sends, recvs = xs, [np.full(c, np.nan, np.float32) for _ in range(n)]
            ret = recvs
        keep.append((sends, recvs))
        for r in range(n):
            sp[i * n + r] = None if sends[r] is None else sends[r].ctypes.data
            rp[i * n + r] = None if recvs[r] is None else recvs[r].ctypes.data
        outs.append(ret)
    steps = ctypes.c_uint64()
    rc = load().mnccl_sim_all_collectives(n, k, colls, scheds, counts, roots, sp, rp, 4, vc, vs, vr, op, slice_bytes,
                                          min_slice, channels, slots, seed, ctypes.byref(steps))
    if rc == -1:
        raise RuntimeError("simulated protocol deadlocked")
    if rc != 0:
        raise ValueError(f"bad simulator arguments (rc={rc})")
    for i, fulls, untouched in checks:
        for f in fulls:
            assert np.all(f[:GUARD] == FILL) and np.all(f[-GUARD:] == FILL), f"call {i}: guard bytes were written"
        for buf, was, what in untouched:
            assert np.array_equal(buf, was), f"call {i}: {what} was written"
    return outs
