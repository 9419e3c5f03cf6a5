"""Rank processes for the GPU tests of ncclSend / ncclRecv into registered windows (one process = one
rank; placement and spawning are tests/gpu_workers.py's).

Every rank owns three device buffers: the WINDOW (registered on the communicator), a PLAIN buffer of
the same size that is never registered, and a buffer its sends read from.  A recv's range is taken
from the window or from the plain buffer, 16-byte aligned plus an optional 2-byte offset, with at
least GUARD fill bytes on both sides; the rank keeps the image both buffers must have, and after every
step compares BOTH whole buffers with it -- so the payloads are exact, the guards on both sides of
every recv range are unchanged, and the rest of the window is untouched.  The message rank src sends
to rank dst is p2p_workers.msg(seed, src, dst, tag, nbytes): each end computes it alone.  All
transfers are ncclFloat16 elements, so any even byte count and offset can be asked for.
"""
import ctypes
import os
import time
import traceback

import numpy as np

from gpu_workers import compare, make_inputs, testkern, use_rank_device
from p2p_workers import msg

FILL, GUARD = 0xAB, 64
WB = 1 << 19          # bytes of the window and of the plain buffer
ARENA = WB // 2       # recv ranges come from the lower half; the upper half serves the window all-reduce
AR_SEND, AR_RECV = WB // 2, WB // 2 + (WB // 4)


def op(kind, peer, nbytes, tag=0, where="win", mis=0, direct=None):
    """One operation: "send" | "recv", the peer, the byte count, a tag that tells the messages of one
    pair apart; a recv's buffer ("win" | "plain"), its 2-byte misalignment, and whether the library is
    expected to post it direct (default: it lies in the window)."""
    return dict(kind=kind, peer=peer, nbytes=nbytes, tag=tag, where=where, mis=mis,
                direct=(where == "win") if direct is None else direct)


class Rank:
    def __init__(self, rank, n, port, env):
        os.environ.update(env)
        os.environ["MINI_NCCL_PORT"] = str(port)
        import hip_rt
        import mini_nccl as M
        self.hip, self.M, self.rank, self.n = hip_rt, M, rank, n
        use_rank_device(rank)
        self.comm = M.Comm(n, rank, "127.0.0.1")
        self.st = hip_rt.Stream()
        self.bufs = {"win": hip_rt.DeviceBuffer(WB, fresh=True), "plain": hip_rt.DeviceBuffer(WB, fresh=True)}
        self.send = hip_rt.DeviceBuffer(WB, fresh=True)
        self.want = {k: np.full(WB, FILL, np.uint8) for k in self.bufs}
        self.at = {"win": 0, "plain": 0, "send": 0}
        for b in self.bufs.values():
            b.fill_byte(FILL)
        self.handle = self.comm.register(self.bufs["win"].ptr, WB)

    def take(self, where, payload, mis=0):
        """A recv range of payload.size bytes that must hold `payload` after the step: its pointer."""
        off = (self.at[where] + GUARD + 15) // 16 * 16 + mis
        self.at[where] = off + payload.size
        assert self.at[where] + GUARD <= ARENA
        self.want[where][off:off + payload.size] = payload
        return self.bufs[where].ptr + off, off

    def put_send(self, payload, mis=0):
        off = (self.at["send"] + 15) // 16 * 16 + mis
        self.at["send"] = off + payload.size
        assert self.at["send"] <= WB
        self.send.upload(payload, off)
        return self.send.ptr + off

    def bad(self):
        """Bytes of the window and of the plain buffer that differ from their images."""
        return sum(int((b.download(np.uint8, WB) != self.want[k]).sum()) for k, b in self.bufs.items())

    def counters(self):
        ci = self.comm.info()
        return {"recvs": ci["p2p_direct_recvs"], "sends": ci["p2p_direct_sends"], "windows": ci["windows"],
                "last_algo": ci["last_algo"], "async": self.comm.async_error()}

    def issue(self, bufs, grouped):
        M, rcs = self.M, []
        if grouped:
            M.group_start()
        for o, ptr in bufs:
            fn = self.comm.send if o["kind"] == "send" else self.comm.recv
            rcs.append(fn(ptr, o["nbytes"] // 2, M.ncclFloat16, o["peer"], self.st.handle))
        if grouped:
            rcs.append(M.group_end())
        return rcs

    def prepare(self, launches, seed):
        self.at["send"] = 0
        out = []
        for launch in launches:
            bufs = []
            for o in launch["ops"]:
                if o["kind"] == "send":
                    ptr = self.put_send(msg(seed, self.rank, o["peer"], o["tag"], o["nbytes"]), o["mis"])
                else:
                    ptr = self.take(o["where"], msg(seed, o["peer"], self.rank, o["tag"], o["nbytes"]), o["mis"])[0]
                bufs.append((o, ptr))
            out.append((bufs, launch.get("group", len(bufs) != 1)))
        return out

    def close(self):
        self.st.destroy()
        rc = self.comm.destroy()
        for b in list(self.bufs.values()) + [self.send]:
            b.free()
        return rc


def _p2p_step(R, step, barrier):
    prepared = R.prepare(step["p2p"].get(R.rank, []), step["seed"])
    R.hip.sync()
    barrier.wait(120)
    rcs = [R.issue(bufs, grouped) for bufs, grouped in prepared]
    R.st.sync()
    return dict(R.counters(), rcs=rcs, bad=R.bad())


def _ar_step(R, step, barrier):
    """One fp32 all-reduce against the oracle: forced to the ring on buffers of its own ("ring"), or
    with send and recv inside the window at the same offsets on every rank ("win")."""
    import oracle_api as O
    hip, M, n, count = R.hip, R.M, R.n, step["count"]
    xs = make_inputs(n, count, "f32", step["seed"], False)
    exp = O.allreduce(xs, "f32", "sum")[R.rank]
    if step["ar"] == "win":
        w = R.bufs["win"]
        w.upload(xs[R.rank], AR_SEND)
        R.want["win"][AR_SEND:AR_SEND + count * 4] = xs[R.rank].view(np.uint8)
        sp, rp, algo = w.ptr + AR_SEND, w.ptr + AR_RECV, M.ALGO_AUTO
    else:
        a, b = hip.DeviceBuffer(count * 4), hip.DeviceBuffer(count * 4)
        a.upload(xs[R.rank])
        sp, rp, algo = a.ptr, b.ptr, M.ALGO_RING
    hip.sync()
    barrier.wait(120)
    R.comm.set_algo(algo)
    rc = R.comm.all_reduce(sp, rp, count, M.ncclFloat, M.ncclSum, R.st.handle)
    R.st.sync()
    R.comm.set_algo(M.ALGO_AUTO)
    if step["ar"] == "win":
        got = R.bufs["win"].download(np.float32, count, AR_RECV)
        R.want["win"][AR_RECV:AR_RECV + count * 4] = exp.view(np.uint8)  # the image follows a correct result
    else:
        got = b.download(np.float32, count)
        a.free()
        b.free()
    return dict(R.counters(), rcs=[[rc]], bad=compare(got, exp, "f32", True)[0] + R.bad())


def _registration_step(R, step, barrier):
    """Collective: deregister the window, or register the same buffer again."""
    barrier.wait(120)
    if step["reg"] == "off":
        R.comm.deregister(R.handle)
    else:
        R.handle = R.comm.register(R.bufs["win"].ptr, WB)
    return dict(R.counters(), rcs=[[0]], bad=R.bad())


def _graph_step(R, step, barrier):
    """n = 2: group{send -> peer, recv <- peer into the window} captured once and replayed with new
    payloads, the recv range refilled before every replay."""
    hip, M, peer, nb = R.hip, R.M, 1 - R.rank, step["nbytes"]
    R.at["send"] = 0
    sptr = R.put_send(msg(step["seed"], R.rank, peer, 0, nb))
    rptr, roff = R.take("win", np.full(nb, FILL, np.uint8))
    ops = [(op("send", peer, nb), sptr), (op("recv", peer, nb), rptr)]
    hip.sync()
    barrier.wait(120)
    rcs = []
    g = hip.Graph(R.st, lambda: rcs.extend(R.issue(ops, True)))
    res = dict(R.counters(), capture_rcs=list(rcs), bad_after_capture=R.bad(), bad=[], sends_after=[])
    for k in range(step["replays"] if rcs == [0, 0, 0] else 0):
        seed = step["seed"] + 1 + k
        R.send.upload(msg(seed, R.rank, peer, 0, nb), sptr - R.send.ptr)
        R.bufs["win"].upload(np.full(nb, FILL, np.uint8), roff)
        R.want["win"][roff:roff + nb] = msg(seed, peer, R.rank, 0, nb)
        hip.sync()
        barrier.wait(120)
        g.launch()
        R.st.sync()
        res["bad"].append(R.bad())
        res["sends_after"].append(R.counters()["sends"])
    g.destroy()
    res.update(R.counters())
    res["rcs"] = [rcs]
    return res


def _consumer_step(R, step, barrier):
    """n = 2: the recv range is first read by an ordinary kernel (its lines sit in this GPU's L2), then
    the group runs and an ordinary kernel copies the range with plain loads right behind the call on
    the same stream; the copy must hold the message."""
    hip, peer, nb = R.hip, 1 - R.rank, step["nbytes"]
    K = testkern()
    seen, word = hip.DeviceBuffer(nb), hip.DeviceBuffer(256)
    bad, rcs = [], []
    for k in range(step["calls"]):
        seed = step["seed"] + k
        R.at["send"] = 0
        payload = msg(seed, peer, R.rank, k, nb)
        sptr = R.put_send(msg(seed, R.rank, peer, k, nb))
        rptr, _ = R.take("win", payload)
        seen.fill_byte(0)
        hip.sync()
        barrier.wait(120)
        vp, h = ctypes.c_void_p, ctypes.c_void_p(R.st.handle)
        hip.check(K.mnccl_test_touch(vp(rptr), nb, vp(word.ptr), h), "touch")
        rcs.append(R.issue([(op("send", peer, nb), sptr), (op("recv", peer, nb), rptr)], True))
        hip.check(K.mnccl_test_copy(vp(seen.ptr), vp(rptr), nb, h), "copy")
        R.st.sync()
        bad.append(int((seen.download(np.uint8, nb) != payload).sum()) + R.bad())
    seen.free()
    word.free()
    return dict(R.counters(), rcs=rcs, bad=sum(bad))


def _mismatch_step(R, step, barrier):
    """n = 2: rank 0 sends step["send"] bytes, rank 1 receives step["recv"] bytes into the window.  The
    recv range and its guards must stay fill bytes (the image is not updated)."""
    hip, M = R.hip, R.M
    R.at["send"] = 0
    if R.rank == 0:
        o, ptr = op("send", 1, step["send"]), R.put_send(msg(step["seed"], 0, 1, 0, step["send"]))
    else:
        o = op("recv", 0, step["recv"], where=step["where"])
        ptr = R.take(step["where"], np.full(step["recv"], FILL, np.uint8))[0]
    hip.sync()
    barrier.wait(120)
    t0 = time.time()
    rc = R.issue([(o, ptr)], False)
    R.st.sync()
    secs = time.time() - t0
    res = dict(R.counters(), rcs=[rc], secs=secs, bad=R.bad())
    res["again"] = R.issue([(o, ptr)], False)  # sticky
    res["async_again"] = R.comm.async_error()
    return res


STEPS = {"p2p": _p2p_step, "ar": _ar_step, "reg": _registration_step, "graph": _graph_step,
         "consume": _consumer_step, "mismatch": _mismatch_step}


def window_p2p_rank(rank, n, port, steps, env, out_q, barrier=None):
    """Run `steps` on one communicator with one registered window, every step checked.  A step is a
    dict with a "seed" and one of: "p2p" {rank: [launch]} (a launch is {"ops": [op(...)], "group":
    bool}); "ar" "ring" | "win" with "count"; "reg" "off" | "on"; "graph"; "consume"; "mismatch"."""
    try:
        R = Rank(rank, n, port, env)
        results = []
        for step in steps:
            kind = next(k for k in STEPS if k in step)
            results.append(STEPS[kind](R, step, barrier))
        info = R.comm.info()
        out_q.put((rank, {"results": results, "info": info, "destroy": R.close()}))
    except Exception:
        out_q.put((rank, {"error": traceback.format_exc()}))
