"""ctypes front end of the point-to-point simulator (csrc/sim.cpp mnccl_sim_p2p) and of the exported
point-to-point geometry (csrc/schedule.h p2p_pipes and the slice map).

A run is a list of phases.  A point-to-point phase is {rank: [launch, ...]}: a launch is a list of
operations ("send" | "recv", peer, buffer) -- one group, or one ungrouped call -- and every rank runs
its launches in order, independently of the other ranks.  A collective phase is ("ar", schedule,
[inputs per rank]): one fp32 all-reduce on the same communicator state.  Buffers are numpy uint8
arrays owned by the caller: sends are read, recvs written in place.
"""
import ctypes

import numpy as np

import sim_api

RING, READ = 0, 2
_ready = False


def load():
    global _ready
    L = sim_api.load()
    if not _ready:
        vp, u64, i, P = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.POINTER
        L.mnccl_resident_cap.argtypes = [i, i, i, i]
        L.mnccl_p2p_pipes.argtypes = [i, i, i, i, i]
        L.mnccl_p2p_msg_pipes.argtypes = [u64, u64, i]
        L.mnccl_p2p_pipe_msgs.argtypes = [u64, u64, i, i]
        L.mnccl_p2p_pipe_msgs.restype = u64
        L.mnccl_p2p_max_group_ops.argtypes = []
        L.mnccl_sim_p2p.argtypes = [i, i, i, u64, i, i, P(i), P(i), P(u64), P(vp), P(vp), i, i, P(i), P(i), P(i), P(i),
                                    P(i), P(vp), P(u64), u64, P(u64), P(u64)]
        _ready = True
    return L


def run(n, phases, channels=2, slots=2, slot_bytes=1024, pipes=2, seed=0):
    """Runs `phases` on one simulated communicator.  Returns (outs, tx, rx): outs[i] is the list of
    the all-reduce's per-rank results for a collective phase (None for a point-to-point phase);
    tx / rx are the final counters, arrays [rank][peer][pipeline].  Raises RuntimeError on no
    progress (a deadlock), ValueError on bad arguments or a group p2p.h refuses."""
    L = load()
    nph = len(phases)
    coll = (ctypes.c_int * max(nph, 1))()
    sched = (ctypes.c_int * max(nph, 1))()
    count = (ctypes.c_uint64 * max(nph, 1))()
    csend = (ctypes.c_void_p * max(nph * n, 1))()
    crecv = (ctypes.c_void_p * max(nph * n, 1))()
    outs, keep = [], []
    ops = []  # (phase, rank, launch, send, peer, pointer, bytes)
    for ph, phase in enumerate(phases):
        if isinstance(phase, dict):
            coll[ph] = -1
            outs.append(None)
            for r in sorted(phase):
                for li, launch in enumerate(phase[r]):
                    for kind, peer, buf in launch:
                        assert buf.dtype == np.uint8 and buf.flags["C_CONTIGUOUS"]
                        keep.append(buf)
                        ops.append((ph, r, li, 1 if kind == "send" else 0, peer, buf.ctypes.data, buf.size))
        else:
            kind, s, xs = phase
            assert kind == "ar" and len(xs) == n
            coll[ph], sched[ph], count[ph] = 0, s, xs[0].size
            res = [np.zeros_like(x) for x in xs]
            for r in range(n):
                x = np.ascontiguousarray(xs[r], dtype=np.float32)
                keep.append(x)
                csend[ph * n + r] = x.ctypes.data
                crecv[ph * n + r] = res[r].ctypes.data
            outs.append(res)
    k = len(ops)
    col = lambda j, t: (t * max(k, 1))(*[o[j] for o in ops])
    C = ctypes
    ctr = (C.c_uint64 * (2 * n * n * channels))()
    steps = C.c_uint64()
    rc = L.mnccl_sim_p2p(n, channels, slots, slot_bytes, pipes, nph, coll, sched, count, csend, crecv, 0, k,
                         col(0, C.c_int), col(1, C.c_int), col(2, C.c_int), col(3, C.c_int), col(4, C.c_int),
                         col(5, C.c_void_p), col(6, C.c_uint64), seed, ctr, C.byref(steps))
    if rc == -1:
        raise RuntimeError("simulated point-to-point run made no progress (deadlock)")
    if rc != 0:
        raise ValueError(f"mnccl_sim_p2p: {rc}")
    a = np.array(list(ctr), dtype=np.uint64).reshape(2, n, n, channels)
    return outs, a[0], a[1]
