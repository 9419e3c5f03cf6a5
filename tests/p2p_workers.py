"""Rank processes for the ncclSend / ncclRecv GPU tests (one process = one rank; placement and spawning
are tests/gpu_workers.py's).

The expected result of a transfer is its bytes.  msg(seed, src, dst, tag, nbytes) is the message rank
src sends to rank dst -- seeded random BYTES, so every bit pattern crosses and each end computes what
it sends and what it must receive without the other's buffers.  Every buffer of every operation has
256 guard bytes behind it (and its offset's bytes in front): after every step each recv holds exactly
its message, each send is unchanged, and all guards are.
"""
import os
import threading
import traceback

import numpy as np

from coll_workers import GUARD, _info_fields
from gpu_workers import make_inputs, compare, use_rank_device

FILL = 0xAB
MAX_GROUP_OPS = 64  # csrc/p2p.h kMaxGroupOps (test_p2p_cpu.py compares it with the library's)


def msg(seed, src, dst, tag, nbytes):
    return np.frombuffer(np.random.default_rng([seed, src, dst, tag]).bytes(nbytes), np.uint8)


def op(kind, peer, dtype="f32", count=1, tag=0, off=0, mem="device"):
    """One operation of a launch: "send" | "recv", the peer, datatype and element count, a tag that
    tells the messages of one pair apart, the buffer's byte offset (a misaligned base) and placement."""
    return dict(kind=kind, peer=peer, dtype=dtype, count=count, tag=tag, off=off, mem=mem)


class _Buf:
    """One operation's buffer: [off bytes][payload][GUARD], FILL outside the payload."""

    def __init__(self, hip_rt, o, rank, seed):
        import oracle_api as O
        self.o = o
        self.code, npd = O.DTYPES[o["dtype"]]
        self.nb = o["count"] * np.dtype(npd).itemsize
        self.off = o["off"]
        self.total = self.off + self.nb + GUARD
        self.buf = hip_rt.buffer(o["mem"], self.total)
        src, dst = (rank, o["peer"]) if o["kind"] == "send" else (o["peer"], rank)
        self.want = np.full(self.total, FILL, np.uint8)
        self.want[self.off:self.off + self.nb] = msg(seed, src, dst, o["tag"], self.nb)
        first = self.want if o["kind"] == "send" else np.full(self.total, FILL, np.uint8)
        self.buf.upload(first)
        self.ptr = self.buf.ptr + self.off

    def bad(self):
        got = self.buf.download(np.uint8, self.total)
        return int((got != self.want).sum())

    def free(self):
        self.buf.free()


def run_launch(M, comm, bufs, grouped, handle):
    """One launch: its operations inside one group, or its single operation ungrouped.  Returns the
    result codes of the calls and, grouped, ncclGroupEnd's as the last one."""
    rcs = []
    if grouped:
        M.group_start()
    for b in bufs:
        fn = comm.send if b.o["kind"] == "send" else comm.recv
        rcs.append(fn(b.ptr, b.o["count"], b.code, b.o["peer"], handle))
    if grouped:
        rcs.append(M.group_end())
    return rcs


def _p2p_step(hip_rt, M, comm, step, rank, stream, barrier):
    launches = step["launches"].get(rank, [])
    seed = step.get("seed", 1)
    bufs = [[_Buf(hip_rt, o, rank, seed) for o in launch["ops"]] for launch in launches]
    hip_rt.sync()
    if barrier is not None:
        barrier.wait(120)
    rcs = [run_launch(M, comm, bs, launch.get("group", len(bs) != 1), stream.handle) for launch, bs in zip(launches, bufs)]
    stream.sync()
    res = {"rcs": rcs, "bad": sum(b.bad() for bs in bufs for b in bs), "idle": not launches}
    res.update(_info_fields(comm))
    for bs in bufs:
        for b in bs:
            b.free()
    return res


def _ar_step(hip_rt, M, comm, step, rank, n, stream, barrier):
    import oracle_api as O
    count, seed = step["count"], step.get("seed", 1)
    xs = make_inputs(n, count, "f32", seed, False)
    exp = O.allreduce(xs, "f32", "sum")[rank]
    send, recv = hip_rt.DeviceBuffer(count * 4), hip_rt.DeviceBuffer(count * 4)
    send.upload(xs[rank])
    hip_rt.sync()
    if barrier is not None:
        barrier.wait(120)
    comm.set_algo(step["algo"])
    rc = comm.all_reduce(send.ptr, recv.ptr, count, M.ncclFloat, M.ncclSum, stream.handle)
    stream.sync()
    res = {"rcs": [[rc]], "bad": compare(recv.download(np.float32, count), exp, "f32", True)[0], "idle": False}
    res.update(_info_fields(comm))
    comm.set_algo(M.ALGO_AUTO)
    send.free()
    recv.free()
    return res


def p2p_rank(rank, n, port, steps, env, out_q, barrier=None):
    """Run `steps` on one communicator, every step checked.  A step is {"launches": {rank: [launch]}}
    -- a launch is {"ops": [op(...)], "group": bool (default: more than one operation)}; a rank with
    no launches makes no call at all in that step -- or {"ar": True, "algo", "count"}: one fp32
    all-reduce against the oracle."""
    try:
        os.environ.update(env)
        os.environ["MINI_NCCL_PORT"] = str(port)
        import hip_rt
        import mini_nccl as M
        use_rank_device(rank)
        comm = M.Comm(n, rank, "127.0.0.1")
        stream = hip_rt.Stream()
        results = []
        for step in steps:
            if step.get("ar"):
                results.append(_ar_step(hip_rt, M, comm, step, rank, n, stream, barrier))
            else:
                results.append(_p2p_step(hip_rt, M, comm, step, rank, stream, barrier))
        stream.destroy()
        info = comm.info()
        out_q.put((rank, {"results": results, "destroy": comm.destroy(), "info": info}))
    except Exception:
        out_q.put((rank, {"error": traceback.format_exc()}))


def _exchange(hip_rt, M, comm, rank, n, stream, seed, count=4099):
    """group{send -> r + 1, recv <- r - 1}, checked: (result codes, mismatching bytes)."""
    bs = [_Buf(hip_rt, op("send", (rank + 1) % n, count=count, tag=7), rank, seed),
          _Buf(hip_rt, op("recv", (rank - 1) % n, count=count, tag=7), rank, seed)]
    hip_rt.sync()
    rcs = run_launch(M, comm, bs, True, stream.handle)
    stream.sync()
    bad = sum(b.bad() for b in bs)
    for b in bs:
        b.free()
    return rcs, bad


def graph_rank(rank, n, port, env, count, replays, out_q, barrier=None):
    """A grouped exchange with the other rank captured ONCE into a HIP graph (the buffers hold a
    first seed's bytes, which no replay expects) and replayed with new send contents and a refilled
    recv before every replay; then one eager exchange."""
    try:
        os.environ.update(env)
        os.environ["MINI_NCCL_PORT"] = str(port)
        import hip_rt
        import mini_nccl as M
        use_rank_device(rank)
        comm = M.Comm(n, rank, "127.0.0.1")
        st = hip_rt.Stream()
        peer, nb = 1 - rank, count * 4
        send, recv = hip_rt.DeviceBuffer(nb + GUARD), hip_rt.DeviceBuffer(nb + GUARD)

        def prepare(seed):
            recv.fill_byte(FILL)
            send.fill_byte(FILL)
            send.upload(msg(seed, rank, peer, 0, nb))
            hip_rt.sync()
            if barrier is not None:
                barrier.wait(120)

        def check(seed):
            s, r = send.download(np.uint8, nb + GUARD), recv.download(np.uint8, nb + GUARD)
            return int((r[:nb] != msg(seed, peer, rank, 0, nb)).sum() + (s[:nb] != msg(seed, rank, peer, 0, nb)).sum() +
                       (r[nb:] != FILL).sum() + (s[nb:] != FILL).sum())

        prepare(300)
        rcs = []

        def issue():
            M.group_start()
            rcs.append(comm.send(send.ptr, count, M.ncclFloat, peer, st.handle))
            rcs.append(comm.recv(recv.ptr, count, M.ncclFloat, peer, st.handle))
            rcs.append(M.group_end())

        g = hip_rt.Graph(st, issue)
        out = {"capture_rc": rcs, "captured_algo": comm.info()["last_algo"], "bad": []}
        for k in range(replays if rcs == [0, 0, 0] else 0):
            prepare(301 + k)
            g.launch()
            st.sync()
            out["bad"].append(check(301 + k))
        g.destroy()
        prepare(400)
        out["eager_rc"], out["eager_bad"] = _exchange(hip_rt, M, comm, rank, n, st, 401)
        out.update(_info_fields(comm))
        send.free()
        recv.free()
        st.destroy()
        out["destroy"] = comm.destroy()
        out_q.put((rank, out))
    except Exception:
        out_q.put((rank, {"error": traceback.format_exc()}))


def threaded_ranks_proc(n, port, env, count, out_q):
    """n ranks as threads of ONE process on one GPU, one group each (a ring shift): the group state
    is per thread, so the threads' groups do not mix.  Every allocation, upload and download happens
    between barriers while no kernel runs (gpu_workers.threaded_ranks_proc's rule)."""
    try:
        os.environ.update(env)
        os.environ["MINI_NCCL_PORT"] = str(port)
        import hip_rt
        import mini_nccl as M
        bar = threading.Barrier(n)
        out = {}

        def rank_main(r):
            try:
                hip_rt.set_device(0)
                comm = M.Comm(n, r, "127.0.0.1")
                st = hip_rt.Stream()
                res = []
                for k in range(2):
                    bs = [_Buf(hip_rt, op("send", (r + 1) % n, count=count, tag=k), r, 50 + k),
                          _Buf(hip_rt, op("recv", (r - 1) % n, count=count, tag=k), r, 50 + k)]
                    hip_rt.sync()
                    bar.wait(120)  # every thread prepared: no copy / memset / free from here on
                    rcs = run_launch(M, comm, bs, True, st.handle)
                    st.sync()
                    bar.wait(120)  # every thread's kernel done
                    res.append({"rcs": rcs, "bad": sum(b.bad() for b in bs)})
                    for b in bs:
                        b.free()
                    bar.wait(120)
                info = _info_fields(comm)
                st.destroy()
                out[r] = dict(info, results=res, destroy=comm.destroy())
            except Exception:
                out[r] = {"error": traceback.format_exc()}
                bar.abort()

        ts = [threading.Thread(target=rank_main, args=(r,)) for r in range(n)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        out_q.put((0, {"ranks": out}))
    except Exception:
        out_q.put((0, {"error": traceback.format_exc()}))


def one_rank(port, env, out_q):
    """nranks == 1: only the self pair exists.  group{send -> 0, recv <- 0} copies (f16 from an odd
    2-byte offset, then f32); a send to rank 0 alone is ncclInvalidUsage, ungrouped and grouped; a
    pair of different sizes is ncclInvalidUsage; the communicator still copies afterwards."""
    try:
        os.environ.update(env)
        os.environ["MINI_NCCL_PORT"] = str(port)
        import hip_rt
        import mini_nccl as M
        use_rank_device(0)
        comm = M.Comm(1, 0, "127.0.0.1")
        st = hip_rt.Stream()
        out = {"rcs": [], "bad": []}

        def pair(dtype, count, off, recv_count=None, alone=False, grouped=True):
            bs = [_Buf(hip_rt, op("send", 0, dtype, count, off=off), 0, 60)]
            if not alone:
                bs.append(_Buf(hip_rt, op("recv", 0, dtype, recv_count or count), 0, 60))
            hip_rt.sync()
            rcs = run_launch(M, comm, bs, grouped, st.handle)
            st.sync()
            if rcs[-1] != 0 and not alone:  # refused: nothing may have been written
                bs[1].want[:] = FILL
            out["rcs"].append(rcs)
            out["bad"].append(sum(b.bad() for b in bs))
            for b in bs:
                b.free()

        pair("f16", 4101, 2)
        pair("f32", 70001, 0)
        pair("f32", 5, 0, alone=True, grouped=False)
        pair("f32", 5, 0, alone=True)
        pair("f32", 300, 0, recv_count=301)
        pair("f32", 4099, 0)
        out.update(_info_fields(comm))
        st.destroy()
        out["destroy"] = comm.destroy()
        out_q.put((0, out))
    except Exception:
        out_q.put((0, {"error": traceback.format_exc()}))


def errors_rank(rank, n, port, env, scenario, out_q, barrier=None):
    """The calls a live communicator must refuse (n = 2, the same scenario on both ranks, so nobody
    waits for a refused call), each followed by a correct exchange:
      peer_range -- peer == nranks: ncclInvalidArgument;
      self       -- peer == rank ungrouped: ncclInvalidUsage;
      overlap    -- two recvs of one group overlapping by one element: ncclInvalidArgument at the second
                    call and from ncclGroupEnd, nothing launched;
      stream     -- a second stream inside a group: ncclInvalidUsage at that call and from ncclGroupEnd;
      pageable   -- a pageable host buffer: ncclInvalidArgument;
      pinned     -- pinned host buffers on both ends: succeeds, exact;
      too_many   -- kMaxGroupOps + 1 operations: ncclInvalidUsage at the last call and from ncclGroupEnd."""
    try:
        os.environ.update(env)
        os.environ["MINI_NCCL_PORT"] = str(port)
        import hip_rt
        import mini_nccl as M
        use_rank_device(rank)
        comm = M.Comm(n, rank, "127.0.0.1")
        st, st2 = hip_rt.Stream(), hip_rt.Stream()
        peer, F, h = 1 - rank, M.ncclFloat, st.handle
        a, b = hip_rt.DeviceBuffer(1 << 16), hip_rt.DeviceBuffer((1 << 16) + GUARD)
        b.fill_byte(FILL)
        hip_rt.sync()
        if barrier is not None:
            barrier.wait(120)
        out = {"bad": 0}
        if scenario == "peer_range":
            rcs = [comm.send(a.ptr, 16, F, n, h), comm.recv(b.ptr, 16, F, -1, h)]
        elif scenario == "self":
            rcs = [comm.send(a.ptr, 16, F, rank, h), comm.recv(b.ptr, 16, F, rank, h)]
        elif scenario == "overlap":
            M.group_start()
            rcs = [comm.recv(b.ptr, 16, F, peer, h), comm.recv(b.ptr + 60, 16, F, peer, h), comm.send(a.ptr, 16, F, peer, h)]
            rcs.append(M.group_end())
        elif scenario == "stream":
            M.group_start()
            rcs = [comm.send(a.ptr, 16, F, peer, h), comm.recv(b.ptr, 16, F, peer, st2.handle)]
            rcs.append(M.group_end())
        elif scenario == "pageable":
            p = hip_rt.PageableBuffer(4096)
            rcs = [comm.send(p.ptr, 16, F, peer, h), comm.recv(p.ptr, 16, F, peer, h)]
            p.free()
        elif scenario == "pinned":
            bs = [_Buf(hip_rt, op("send", peer, count=4099, mem="pinned"), rank, 80),
                  _Buf(hip_rt, op("recv", peer, count=4099, mem="pinned"), rank, 80)]
            rcs = run_launch(M, comm, bs, True, h)
            st.sync()
            out["bad"] += sum(x.bad() for x in bs)
            for x in bs:
                x.free()
        else:
            k = MAX_GROUP_OPS
            M.group_start()
            rcs = [comm.send(a.ptr + 64 * i, 4, F, peer, h) if i % 2 == 0 else comm.recv(b.ptr + 64 * i, 4, F, peer, h)
                   for i in range(k + 1)]
            rcs.append(M.group_end())
            rcs = rcs[:2] + rcs[k - 1:]  # the first two, the last accepted one, the refused one, ncclGroupEnd
        st.sync()
        out["rcs"] = rcs
        out["touched"] = int((b.download(np.uint8, (1 << 16) + GUARD) != FILL).sum())  # a refused call launches nothing
        out["async_after"] = comm.async_error()
        if barrier is not None:
            barrier.wait(120)
        out["next_rc"], nb = _exchange(hip_rt, M, comm, rank, n, st, 81)
        out["bad"] += nb
        out.update(_info_fields(comm))
        a.free()
        b.free()
        st.destroy()
        st2.destroy()
        out["destroy"] = comm.destroy()
        out_q.put((rank, out))
    except Exception:
        out_q.put((rank, {"error": traceback.format_exc()}))
