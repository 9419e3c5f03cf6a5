"""ctypes front end of the simulator's entry point for sequences that include ncclAllToAll
(csrc/sim.cpp mnccl_sim_mixed) and the permutation an all-to-all is.

Any of the six collectives may follow any other, on either schedule, on ONE simulated communicator
state.  An all-to-all's buffers are raw bytes (viewed as fp32 words by the simulator, which only
copies them): seeded random bytes, so NaN payloads, denormals and every bit pattern occur.
"""
import ctypes

import numpy as np

import sim_rooted_api as R

ALLREDUCE, REDUCE_SCATTER, ALLGATHER, BROADCAST, REDUCE, ALLTOALL = 0, 1, 2, 3, 4, 5
RING, READ = R.RING, R.READ
GUARD = 256  # bytes past each recv that must come back unchanged
GUARD_BYTE = 0xA5

_ready = False


def load():
    global _ready
    L = R.load()
    if not _ready:
        vp, u64, i = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int
        L.mnccl_sim_mixed.argtypes = [i, i, ctypes.POINTER(i), ctypes.POINTER(i), ctypes.POINTER(u64), ctypes.POINTER(i),
                                      ctypes.POINTER(vp), ctypes.POINTER(vp), i, u64, u64, i, i, u64,
                                      ctypes.POINTER(u64)]
        _ready = True
    return L


def random_blocks(n, block_bytes, seed):
    """Rank r's send: n blocks of block_bytes seeded random bytes, different per rank and seed."""
    return [np.random.default_rng([seed, r, n, block_bytes]).integers(0, 256, n * block_bytes, dtype=np.uint8)
            for r in range(n)]


def expect(sends):
    """The permutation: block r of rank q's recv is block q of rank r's send."""
    n = len(sends)
    b = sends[0].size // n
    return [np.concatenate([sends[r][q * b:(q + 1) * b] for r in range(n)]) for q in range(n)]


def run(n, calls, op=0, slice_bytes=1024, channels=4, slots=2, seed=0, min_slice=0):
    """calls: a list of (coll, sched, inputs, inplace, root).  An all-to-all's inputs[r] is rank r's
    send as uint8 (n blocks, a multiple of 4 bytes each; inplace and root ignored); its recv gets GUARD
    bytes behind it, and the guard and the send are checked here after the run.  The five other
    collectives take fp32 inputs as sim_rooted_api.run does, except that every rank passes real
    buffers: a Broadcast's non-root send is NULL, a Reduce's non-root recv a scratch buffer.
    Returns each call's per-rank recv contents (an all-to-all's as uint8 without the guard); raises
    RuntimeError on deadlock."""
    k = len(calls)
    colls = (ctypes.c_int * k)(*[c[0] for c in calls])
    scheds = (ctypes.c_int * k)(*[c[1] for c in calls])
    roots = (ctypes.c_int * k)(*[c[4] for c in calls])
    counts = (ctypes.c_uint64 * k)()
    sp = (ctypes.c_void_p * (k * n))()
    rp = (ctypes.c_void_p * (k * n))()
    keep, outs, a2a = [], [], []
    for i, (coll, _, inputs, inplace, root) in enumerate(calls):
        assert len(inputs) == n
        if coll == ALLTOALL:
            nbytes = inputs[0].size
            assert nbytes % (4 * n) == 0
            counts[i] = nbytes // (4 * n)
            sends = [np.array(x, dtype=np.uint8) for x in inputs]
            full = [np.full(nbytes + GUARD, GUARD_BYTE, np.uint8) for _ in range(n)]
            recvs = [f[:nbytes] for f in full]
            a2a.append((i, inputs, sends, full))
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
    rc = load().mnccl_sim_mixed(n, k, colls, scheds, counts, roots, sp, rp, op, slice_bytes, min_slice, channels, slots,
                                seed, ctypes.byref(steps))
    if rc == -1:
        raise RuntimeError("simulated protocol deadlocked")
    if rc != 0:
        raise ValueError(f"bad simulator arguments (rc={rc})")
    for i, inputs, sends, full in a2a:
        for r in range(n):
            assert np.array_equal(sends[r], inputs[r]), f"call {i}: rank {r}'s send was written"
            assert np.all(full[r][-GUARD:] == GUARD_BYTE), f"call {i}: rank {r}'s guard bytes were written"
    return outs
