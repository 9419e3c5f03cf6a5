"""ctypes front end of the simulator's entry point for sequences that include the two rooted
collectives (csrc/sim.cpp mnccl_sim_rooted) and of their ring tables (csrc/schedule.h coll_op with
a root, coll_tx_msgs / coll_rx_msgs, rooted_len).

Any of the five collectives may follow any other, on either schedule, with a root per call, on ONE
simulated communicator state, as on a real communicator.
"""
import ctypes

import numpy as np

import sim_api
import sim_coll_api as S

ALLREDUCE, REDUCE_SCATTER, ALLGATHER, BROADCAST, REDUCE = 0, 1, 2, 3, 4
RING, READ = sim_api.RING, sim_api.READ
SENTINEL = np.float32(-12345.5)

_ready = False
last_spares = []


def load():
    global _ready
    L = S.load()
    if not _ready:
        vp, u64, i = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int
        L.mnccl_sim_rooted.argtypes = [i, i, ctypes.POINTER(i), ctypes.POINTER(i), ctypes.POINTER(u64), ctypes.POINTER(i),
                                       ctypes.POINTER(vp), ctypes.POINTER(vp), i, u64, u64, i, i, u64,
                                       ctypes.POINTER(u64)]
        L.mnccl_coll_op_rooted.argtypes = [i, i, i, i, i, ctypes.POINTER(i)]
        L.mnccl_coll_tx_msgs.argtypes = [i, i, i, i]
        L.mnccl_coll_rx_msgs.argtypes = [i, i, i, i]
        L.mnccl_rooted_len.argtypes = [u64] * 5
        L.mnccl_rooted_len.restype = u64
        _ready = True
    return L


def coll_op(coll, n, r, k, root):
    """schedule.h coll_op(coll, n, r, k, root) as (kind, chunk, send_msg, recv_msg)."""
    out = (ctypes.c_int * 4)()
    load().mnccl_coll_op_rooted(coll, n, r, k, root, out)
    return tuple(out)


def tx_msgs(coll, n, r, root):
    return load().mnccl_coll_tx_msgs(coll, n, r, root)


def rx_msgs(coll, n, r, root):
    return load().mnccl_coll_rx_msgs(coll, n, r, root)


def rooted_len(total_bytes, chunk_off, chunk_bytes, slice_bytes, s):
    return load().mnccl_rooted_len(total_bytes, chunk_off, chunk_bytes, slice_bytes, s)


def run(n, calls, op=0, slice_bytes=1024, channels=4, slots=2, seed=0, min_slice=0):
    """calls: a list of (coll, sched, inputs, inplace, root).  The three unrooted collectives as
    sim_coll_api.run (root ignored).  Broadcast / Reduce: inputs[r] is rank r's fp32 send of `count`
    elements; `inplace` is the root's (send == recv there).  A non-root's unused buffer is NULL on
    odd ranks; on even ranks it is a buffer filled with SENTINEL (a Broadcast's send, a Reduce's
    recv), which is returned so the caller can check it came back unchanged.
    Returns each call's per-rank recv contents; for a Reduce, rank r != root's entry is its
    sentinel buffer (None where it passed NULL); raises RuntimeError on deadlock.  last_spares[i][r]:
    the sentinel buffer rank r passed for its unused side in call i (None: NULL, or no unused side)."""
    global last_spares
    last_spares = []
    k = len(calls)
    colls = (ctypes.c_int * k)(*[c[0] for c in calls])
    scheds = (ctypes.c_int * k)(*[c[1] for c in calls])
    roots = (ctypes.c_int * k)(*[c[4] for c in calls])
    counts = (ctypes.c_uint64 * k)()
    sp = (ctypes.c_void_p * (k * n))()
    rp = (ctypes.c_void_p * (k * n))()
    keep, outs = [], []
    for i, (coll, _, inputs, inplace, root) in enumerate(calls):
        assert len(inputs) == n
        xs = [np.array(x, dtype=np.float32) for x in inputs]  # own copies (in place writes them)
        if coll in (BROADCAST, REDUCE):
            c = xs[0].size
            counts[i] = c
            sends, recvs, ret = [], [], []
            last_spares.append([np.full(c, SENTINEL, np.float32) if r % 2 == 0 and r != root else None for r in range(n)])
            for r in range(n):
                spare = last_spares[-1][r]
                if coll == BROADCAST:
                    rv = xs[r] if (r == root and inplace) else np.full(c, np.nan, np.float32)
                    sends.append(xs[r] if r == root else spare)
                    recvs.append(rv)
                    ret.append(rv)
                else:
                    rv = (xs[r] if inplace else np.full(c, np.nan, np.float32)) if r == root else spare
                    sends.append(xs[r])
                    recvs.append(rv)
                    ret.append(rv)
            keep.append((sends, recvs))
            for r in range(n):
                sp[i * n + r] = None if sends[r] is None else sends[r].ctypes.data
                rp[i * n + r] = None if recvs[r] is None else recvs[r].ctypes.data
            outs.append(ret)
            continue
        last_spares.append([None] * n)
        if coll == ALLREDUCE:
            counts[i] = xs[0].size
            recvs = xs if inplace else [np.full_like(x, np.nan) for x in xs]
            sends = xs
        elif coll == REDUCE_SCATTER:
            c = xs[0].size // n
            counts[i] = c
            sends = xs
            recvs = [x[r * c:(r + 1) * c] if inplace else np.full(c, np.nan, np.float32) for r, x in enumerate(xs)]
        else:
            c = xs[0].size
            counts[i] = c
            recvs = [np.full(n * c, np.nan, np.float32) for _ in range(n)]
            if inplace:
                for r in range(n):
                    recvs[r][r * c:(r + 1) * c] = xs[r]
                sends = [recvs[r][r * c:(r + 1) * c] for r in range(n)]
            else:
                sends = xs
        keep.append((sends, recvs))
        for r in range(n):
            sp[i * n + r] = sends[r].ctypes.data
            rp[i * n + r] = recvs[r].ctypes.data
        outs.append(recvs)
    steps = ctypes.c_uint64()
    rc = load().mnccl_sim_rooted(n, k, colls, scheds, counts, roots, sp, rp, op, slice_bytes, min_slice, channels,
                                 slots, seed, ctypes.byref(steps))
    if rc == -1:
        raise RuntimeError("simulated protocol deadlocked")
    if rc != 0:
        raise ValueError(f"bad simulator arguments (rc={rc})")
    return outs
