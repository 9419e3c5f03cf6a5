"""ctypes front end of the simulator's multi-collective entry point (csrc/sim.cpp
mnccl_sim_collective) and of the ring halves' op tables (csrc/schedule.h coll_op).

A sequence of all-reduce / reduce-scatter / all-gather calls runs on ONE simulated communicator
state -- the shared FIFO counters, mailboxes and scratch slots continue from call to call, as on a
real communicator -- with the same schedule.h tables the kernels execute.
"""
import ctypes

import numpy as np

import sim_api

ALLREDUCE, REDUCE_SCATTER, ALLGATHER = 0, 1, 2
RING, ONESHOT, READ, READ_GRID = sim_api.RING, sim_api.ONESHOT, sim_api.READ, sim_api.READ_GRID

_ready = False


def load():
    global _ready
    L = sim_api.load()
    if not _ready:
        vp, u64, i = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int
        L.mnccl_sim_collective.argtypes = [i, i, ctypes.POINTER(i), ctypes.POINTER(i), ctypes.POINTER(u64),
                                           ctypes.POINTER(vp), ctypes.POINTER(vp), i, u64, u64, i, i, u64,
                                           ctypes.POINTER(u64)]
        L.mnccl_coll_num_ops.argtypes = [i, i]
        L.mnccl_coll_msgs_per_iter.argtypes = [i, i]
        L.mnccl_coll_op.argtypes = [i, i, i, i, ctypes.POINTER(i)]
        _ready = True
    return L


def num_ops(coll, n):
    return load().mnccl_coll_num_ops(coll, n)


def msgs_per_iter(coll, n):
    return load().mnccl_coll_msgs_per_iter(coll, n)


def coll_op(coll, n, r, k):
    """schedule.h coll_op(coll, n, r, k) as (kind, chunk, send_msg, recv_msg); coll < 0: ring_op."""
    out = (ctypes.c_int * 4)()
    load().mnccl_coll_op(coll, n, r, k, out)
    return tuple(out)


def run(n, calls, op=0, slice_bytes=1024, channels=4, slots=2, seed=0, min_slice=0):
    """calls: a list of (coll, sched, inputs, inplace) -- inputs[r] is rank r's fp32 send (count
    elements for an all-reduce and an all-gather's chunk, n * count for a reduce-scatter).  Runs
    them in order on one communicator state; returns each call's per-rank recv contents (a
    reduce-scatter's chunk, an all-gather's n chunks, an all-reduce's buffer).  Raises
    RuntimeError on deadlock."""
    k = len(calls)
    colls = (ctypes.c_int * k)(*[c[0] for c in calls])
    scheds = (ctypes.c_int * k)(*[c[1] for c in calls])
    counts = (ctypes.c_uint64 * k)()
    sp = (ctypes.c_void_p * (k * n))()
    rp = (ctypes.c_void_p * (k * n))()
    keep, outs = [], []
    for i, (coll, _, inputs, inplace) in enumerate(calls):
        assert len(inputs) == n
        xs = [np.array(x, dtype=np.float32) for x in inputs]  # own copies (in place writes them)
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
    rc = load().mnccl_sim_collective(n, k, colls, scheds, counts, sp, rp, op, slice_bytes, min_slice, channels, slots,
                                     seed, ctypes.byref(steps))
    if rc == -1:
        raise RuntimeError("simulated protocol deadlocked")
    if rc != 0:
        raise ValueError(f"bad simulator arguments (rc={rc})")
    return outs
