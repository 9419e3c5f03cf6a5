"""ctypes front end of the point-to-point simulator's window form (csrc/sim.cpp mnccl_sim_p2p_win) and of
the pure functions csrc/p2p.h adds for it (slot assignment, the direct / scratch decision, the DEST
record).

A run is sim_p2p_api's list of phases with one more field per operation: ("send" | "recv", peer,
buffer, window) -- window is None (a recv posted "scratch"; every send) or the index of the registered
window the recv's range lies in (posted "direct").  windows[k][q] is rank q's buffer of window k, a
numpy uint8 array; every rank's buffer of one window has the same size.
"""
import ctypes

import numpy as np

import sim_api

_ready = False


def load():
    global _ready
    L = sim_api.load()
    if not _ready:
        vp, u64, i, P = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.POINTER
        L.mnccl_sim_p2p_win.argtypes = [i, i, i, u64, i, i, P(i), P(i), P(u64), P(vp), P(vp), i, i, P(i), P(i), P(i),
                                        P(i), P(i), P(vp), P(u64), P(i), i, P(vp), P(u64), u64, P(u64), P(u64), P(u64)]
        L.mnccl_p2p_win_slots.argtypes = []
        L.mnccl_p2p_win_assign.argtypes = [i, P(ctypes.c_int64), P(i)]
        L.mnccl_p2p_win_assign.restype = None
        L.mnccl_p2p_win_direct.argtypes = [i, i, i]
        L.mnccl_p2p_dest_roundtrip.argtypes = [P(u64), P(u64), P(u64)]
        L.mnccl_p2p_dest_roundtrip.restype = None
        L.mnccl_p2p_dest_tag.argtypes = [u64]
        L.mnccl_p2p_dest_tag.restype = u64
        L.mnccl_p2p_dest_check.argtypes = [i, ctypes.c_uint32, u64, u64, u64, u64, u64]
        L.mnccl_mbox_word.argtypes = [i, i, i, i, i]
        L.mnccl_mbox_word.restype = u64
        _ready = True
    return L


def assign(ops):
    """ops: +id registers window id, -id deregisters it.  The slot each step took or freed (-1: none)."""
    L = load()
    out = (ctypes.c_int * len(ops))()
    L.mnccl_p2p_win_assign(len(ops), (ctypes.c_int64 * len(ops))(*ops), out)
    return list(out)


def roundtrip(tag, direct, slot, off, nbytes):
    """(the record's four mailbox words, the record decoded from them)."""
    L = load()
    words, back = (ctypes.c_uint64 * 4)(), (ctypes.c_uint64 * 5)()
    L.mnccl_p2p_dest_roundtrip((ctypes.c_uint64 * 5)(tag, direct, slot, off, nbytes), words, back)
    return list(words), tuple(back)


def run(n, phases, windows, channels=2, slots=2, slot_bytes=1024, pipes=2, seed=0):
    """Runs `phases` on one simulated communicator with `windows` registered.  Returns (outs, tx, rx,
    direct): sim_p2p_api.run's three, and direct[r] = (recvs rank r posted direct, messages it pushed
    direct).  RuntimeError on no progress, ValueError on bad arguments or a refused group,
    LookupError when a sender refuses a DEST record."""
    L = load()
    C = ctypes
    nph = len(phases)
    coll = (C.c_int * max(nph, 1))()
    sched = (C.c_int * max(nph, 1))()
    count = (C.c_uint64 * max(nph, 1))()
    csend = (C.c_void_p * max(nph * n, 1))()
    crecv = (C.c_void_p * max(nph * n, 1))()
    outs, keep, ops = [], [], []  # ops: (phase, rank, launch, send, peer, pointer, bytes, window)
    for ph, phase in enumerate(phases):
        if isinstance(phase, dict):
            coll[ph] = -1
            outs.append(None)
            for r in sorted(phase):
                for li, launch in enumerate(phase[r]):
                    for kind, peer, buf, win in launch:
                        assert buf.dtype == np.uint8 and buf.flags["C_CONTIGUOUS"]
                        keep.append(buf)
                        ops.append((ph, r, li, 1 if kind == "send" else 0, peer, buf.ctypes.data, buf.size,
                                    -1 if win is None else win))
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
    nwin = len(windows)
    wbase = (C.c_void_p * max(nwin * n, 1))()
    wbytes = (C.c_uint64 * max(nwin, 1))()
    for w, per_rank in enumerate(windows):
        assert len(per_rank) == n and len({b.size for b in per_rank}) == 1
        wbytes[w] = per_rank[0].size
        for q in range(n):
            wbase[w * n + q] = per_rank[q].ctypes.data
    ctr = (C.c_uint64 * (2 * n * n * channels))()
    direct = (C.c_uint64 * (2 * n))()
    steps = C.c_uint64()
    rc = L.mnccl_sim_p2p_win(n, channels, slots, slot_bytes, pipes, nph, coll, sched, count, csend, crecv, 0, k,
                             col(0, C.c_int), col(1, C.c_int), col(2, C.c_int), col(3, C.c_int), col(4, C.c_int),
                             col(5, C.c_void_p), col(6, C.c_uint64), col(7, C.c_int), nwin, wbase, wbytes, seed, ctr,
                             direct, C.byref(steps))
    if rc == -1:
        raise RuntimeError("simulated point-to-point run made no progress (deadlock)")
    if rc == -4:
        raise LookupError("a sender refused the receiver's DEST record")
    if rc != 0:
        raise ValueError(f"mnccl_sim_p2p_win: {rc}")
    a = np.array(list(ctr), dtype=np.uint64).reshape(2, n, n, channels)
    d = [(direct[2 * r], direct[2 * r + 1]) for r in range(n)]
    return outs, a[0], a[1], d
