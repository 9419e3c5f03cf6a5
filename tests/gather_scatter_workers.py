"""Rank processes for the ncclGather / ncclScatter GPU tests (one process = one rank; placement,
spawning and comparison are tests/gpu_workers.py's; the seven other collectives between them run
through the eager runners of tests/rooted_workers.py and tests/alltoall_workers.py).

The expected result is the permutation itself, computed with numpy from the same seeded inputs: a
gather's root holds the ranks' blocks in rank order, a scatter's rank q block q of the root's send.
Blocks are seeded random BYTES (block_bytes): NaN payloads and every other bit pattern occur, and the
comparison is of bytes.  Every buffer sits between GUARD sentinel bytes, before it and after it; a
non-root's unused large buffer is NULL or a sentinel buffer, and all of them must come back unchanged
(GSCall.check).
"""
import ctypes
import os
import time
import traceback

import numpy as np

import alltoall_workers as AW
import rooted_workers as RW
from coll_workers import _info_fields, per_rank
from gpu_workers import testkern, use_rank_device

GUARD = 256
FILL = 0xAB
ESZ = {"f16": 2, "bf16": 2, "f32": 4, "i32": 4, "f64": 8}


def block_bytes(seed, r, nbytes):
    """Rank r's block for `seed` (a gather's send; block r of a scatter's send on the root)."""
    return np.random.default_rng([seed, r]).integers(0, 256, nbytes, dtype=np.uint8)


class _Region:
    """nbytes at a byte offset `off` behind a front guard, with a back guard behind them: in an
    allocation of its own (mem: device / pinned / pageable), or at `at` of a registered window."""

    def __init__(self, hip_rt, nbytes, off, mem="device", window=None, at=0):
        self.hip_rt, self.nbytes, self.span = hip_rt, nbytes, GUARD + off + nbytes + GUARD
        self.owned = window is None
        self.owner = hip_rt.buffer(mem, self.span) if self.owned else window
        self.at = 0 if self.owned else at
        self.lo = self.at + GUARD + off  # the buffer's first byte in the owner
        self.ptr = self.owner.ptr + self.lo

    def fill(self):
        if self.owned:
            self.owner.fill_byte(FILL)
        else:
            self.hip_rt.View(self.owner, self.at, self.span).fill_byte(FILL)

    def upload(self, arr, offset=0):
        self.owner.upload(arr, self.lo + offset)

    def download(self):
        """(the buffer's bytes, the bytes of both guards and the offset padding)"""
        whole = self.owner.download(np.uint8, self.span, self.at)
        a = self.lo - self.at
        return whole[a:a + self.nbytes], np.concatenate([whole[:a], whole[a + self.nbytes:]])

    def free(self):
        if self.owned:
            self.owner.free()


class GSCall:
    """One gather ("ga") / scatter ("sc") on one rank: `count` elements of `dtype` per block.  inplace:
    the root's one-block buffer is block `root` of its large one.  null: a non-root passes NULL for the
    large buffer (otherwise a sentinel buffer).  offset: bytes added to every buffer's base (2: a
    misaligned base).  mem: where the buffers live (device / pinned / pageable).  window: (send
    window, offset, recv window, offset) -- both buffers at fixed places of registered windows."""

    def __init__(self, hip_rt, coll, n, rank, count, dtype="f32", root=0, inplace=False, null=False, offset=0,
                 mem="device", window=None):
        self.coll, self.n, self.rank, self.count, self.dtype, self.root = coll, n, rank, count, dtype, root
        self.b = count * ESZ[dtype]
        self.is_root = rank == root
        self.inplace = inplace and self.is_root
        b, nb = self.b, n * self.b
        big_is_send = coll == "sc"
        sw, so, rw, ro = window if window else (None, 0, None, 0)
        self.big = self.small = None
        if self.is_root or not null:
            self.big = _Region(hip_rt, nb, offset, mem, sw if big_is_send else rw, so if big_is_send else ro)
        if not self.inplace:
            self.small = _Region(hip_rt, b, offset, mem, rw if big_is_send else sw, ro if big_is_send else so)
        self.regions = [x for x in (self.big, self.small) if x is not None]
        small_ptr = self.big.ptr + rank * b if self.inplace else self.small.ptr
        big_ptr = self.big.ptr if self.big is not None else None
        self.send_ptr, self.recv_ptr = (big_ptr, small_ptr) if big_is_send else (small_ptr, big_ptr)

    def prepare(self, seed):
        """Sentinels everywhere, then this call's input; the expected bytes of every buffer after it."""
        n, b, r = self.n, self.b, self.rank
        for x in self.regions:
            x.fill()
        self.exp_big = np.full(n * b, FILL, np.uint8) if self.big is not None else None
        self.exp_small = np.full(b, FILL, np.uint8)
        if self.coll == "ga":
            mine = block_bytes(seed, r, b)
            if self.inplace:
                self.big.upload(mine, r * b)
            else:
                self.small.upload(mine)
                self.exp_small = mine
            if self.is_root:
                self.exp_big = np.concatenate([block_bytes(seed, q, b) for q in range(n)])
        else:
            if self.is_root:
                self.exp_big = np.concatenate([block_bytes(seed, q, b) for q in range(n)])
                self.big.upload(self.exp_big)
            self.exp_small = block_bytes(seed, r, b)

    def issue(self, comm, st):
        import oracle_api as O
        f = comm.gather if self.coll == "ga" else comm.scatter
        return f(self.send_ptr, self.recv_ptr, self.count, O.DTYPES[self.dtype][0], self.root, st.handle)

    def check(self):
        """(bytes that differ from what the call defines, guards and unused buffers included; detail)"""
        bad, detail = 0, ""
        for name, reg, exp in (("large", self.big, self.exp_big), ("one-block", self.small, self.exp_small)):
            if reg is None:
                continue
            got, guards = reg.download()
            d = np.flatnonzero(got != exp)
            g = int((guards != FILL).sum())
            if d.size or g:
                bad += int(d.size) + g
                detail += f" {name} buffer: {d.size} bytes differ" + (f" (first {int(d[0])})" if d.size else "") + \
                          f", {g} guard bytes written;"
        return bad, detail

    def free(self):
        for x in self.regions:
            x.free()


def _open(rank, n, port, env):
    os.environ.update(env)
    os.environ["MINI_NCCL_PORT"] = str(port)
    import hip_rt
    import mini_nccl as M
    use_rank_device(rank)
    return hip_rt, M, M.Comm(n, rank, "127.0.0.1")


def _wait(barrier):
    if barrier is not None:
        barrier.wait(120)


def _gs_case(hip_rt, comm, case, rank, n, st, barrier, rng):
    """One gather / scatter case: coll, dtype, count, root, inplace, null, offset, mem (a value or a
    per-rank list), calls (new bytes every call), skew_ms."""
    call = GSCall(hip_rt, case["coll"], n, rank, case["count"], case.get("dtype", "f32"), case["root"],
                  case.get("inplace", False), case.get("null", False), case.get("offset", 0),
                  per_rank(case.get("mem", "device"), rank))
    bad, detail, rc, algos = 0, "", 0, []
    t0 = time.time()
    for k in range(case.get("calls", 1)):
        call.prepare(case.get("seed", 1) + 1000 * k)
        hip_rt.sync()
        _wait(barrier)
        if case.get("skew_ms"):
            time.sleep(float(rng.uniform(0, case["skew_ms"])) / 1000.0)
        rc = call.issue(comm, st)
        if rc != 0:
            bad = -1
            break
        st.sync()
        algos.append(comm.info()["last_algo"])
        b, d = call.check()
        bad += b
        detail += f" call {k}:{d}" if b else ""
    res = {"case": case, "rc": rc, "bad": bad, "first": -1, "detail": detail, "algos": algos, "secs": time.time() - t0}
    res.update(_info_fields(comm))
    call.free()
    return res


def cases_rank(rank, n, port, cases, env, out_q, barrier=None):
    """Run `cases` on one communicator, every call checked: gathers and scatters (_gs_case) and, between
    them, the other collectives ("ar" / "rs" / "ag" / "bc" / "rd" / "a2a": the cases of
    rooted_workers and alltoall_workers)."""
    try:
        hip_rt, M, comm = _open(rank, n, port, env)
        st = hip_rt.Stream()
        results = []
        for case in cases:
            comm.set_algo(case["algo"])
            rng = np.random.default_rng(case.get("seed", 1) * 97 + rank)
            coll = case["coll"]
            if coll in ("ga", "sc"):
                results.append(_gs_case(hip_rt, comm, case, rank, n, st, barrier, rng))
            else:
                run = AW._a2a_case if coll == "a2a" else RW._rooted_case if coll in ("bc", "rd") else RW._unrooted_case
                results.append(run(comm, case, rank, n, st, barrier, rng))
        st.destroy()
        info = comm.info()
        out_q.put((rank, {"results": results, "destroy": comm.destroy(), "info": info}))
    except Exception:
        out_q.put((rank, {"error": traceback.format_exc()}))


def identities_rank(rank, n, port, env, algo, count, rounds, out_q, barrier=None):
    """On one communicator, `rounds` times with new bytes and another root: gather then scatter from the
    same root returns this rank's input; the root's gather result equals its ncclAllGather result;
    this rank's scatter result equals block `rank` of what ncclBroadcast of the root's send delivers."""
    try:
        hip_rt, M, comm = _open(rank, n, port, env)
        comm.set_algo(algo)
        st = hip_rt.Stream()
        b, nb, F, h = count * 4, n * count * 4, M.ncclFloat, st.handle
        src, back, part = (hip_rt.DeviceBuffer(b) for _ in range(3))
        gath, allg, deal, bcast = (hip_rt.DeviceBuffer(nb) for _ in range(4))
        out = {"rcs": [], "round_trip_bad": [], "gather_vs_allgather": [], "scatter_vs_broadcast": [], "algos": []}
        for k in range(rounds):
            root = (k + 1) % n
            is_root = rank == root
            mine = block_bytes(7000 + k, rank, b)
            src.upload(mine)
            for x in (back, part, gath, allg, deal, bcast):
                x.fill_byte(FILL)
            if is_root:
                deal.upload(np.concatenate([block_bytes(7500 + k, q, b) for q in range(n)]))
            hip_rt.sync()
            _wait(barrier)
            rcs = [comm.gather(src.ptr, gath.ptr if is_root else None, count, F, root, h)]
            a1 = comm.info()["last_algo"]
            rcs.append(comm.scatter(gath.ptr if is_root else None, back.ptr, count, F, root, h))
            a2 = comm.info()["last_algo"]
            rcs.append(comm.all_gather(src.ptr, allg.ptr, count, F, h))
            rcs.append(comm.scatter(deal.ptr if is_root else None, part.ptr, count, F, root, h))
            rcs.append(comm.broadcast(deal.ptr if is_root else None, bcast.ptr, n * count, F, root, h))
            st.sync()
            out["rcs"].append(rcs)
            out["algos"].append((a1, a2))
            out["round_trip_bad"].append(int((back.download(np.uint8, b) != mine).sum()))
            g, a = gath.download(np.uint8, nb), allg.download(np.uint8, nb)
            # (a non-root's gath was never passed: nobody wrote it)
            out["gather_vs_allgather"].append(int((g != a).sum()) if is_root else int((g != FILL).sum()))
            whole = bcast.download(np.uint8, nb)
            out["scatter_vs_broadcast"].append(int((part.download(np.uint8, b) != whole[rank * b:(rank + 1) * b]).sum()))
        out.update(_info_fields(comm))
        for x in (src, back, part, gath, allg, deal, bcast):
            x.free()
        st.destroy()
        out["destroy"] = comm.destroy()
        out_q.put((rank, out))
    except Exception:
        out_q.put((rank, {"error": traceback.format_exc()}))


def consumer_rank(rank, n, port, env, coll, count, rounds, out_q, barrier=None):
    """gpu_workers.cached_consumer_rank's shape for the two kernels' pushes: the buffer the call fills
    -- the root's recv for "ga", every rank's for "sc" -- is first read by an ordinary kernel (its lines
    sit in this GPU's L2), then the call (the peers push into it), and an ordinary kernel copies it
    with plain loads right behind the call on the same stream (MINI_NCCL_BLOCKING=0: no host wait in
    between).  New bytes and another root every round."""
    try:
        hip_rt, M, comm = _open(rank, n, port, env)
        K = testkern()
        comm.set_algo(M.ALGO_READ)
        st = hip_rt.Stream()
        b, nb = count * 4, n * count * 4
        rb = nb if coll == "ga" else b  # the recv's bytes
        send, recv, seen, word = (hip_rt.DeviceBuffer(x) for x in (nb, rb, rb, 256))
        recv.fill_byte(0)
        bad, rcs, algos = [], [], []
        for c in range(rounds):
            root = c % n
            is_root = rank == root
            reads = coll == "sc" or is_root
            blocks = [block_bytes(6000 + c, q, b) for q in range(n)]
            send.upload(np.concatenate(blocks) if coll == "sc" else blocks[rank])
            hip_rt.sync()
            _wait(barrier)
            if reads:
                hip_rt.check(K.mnccl_test_touch(ctypes.c_void_p(recv.ptr), rb, ctypes.c_void_p(word.ptr),
                                                ctypes.c_void_p(st.handle)), "touch")
            if coll == "ga":
                rc = comm.gather(send.ptr, recv.ptr if is_root else None, count, M.ncclFloat, root, st.handle)
            else:
                rc = comm.scatter(send.ptr if is_root else None, recv.ptr, count, M.ncclFloat, root, st.handle)
            if reads:
                hip_rt.check(K.mnccl_test_copy(ctypes.c_void_p(seen.ptr), ctypes.c_void_p(recv.ptr), rb,
                                               ctypes.c_void_p(st.handle)), "copy")
            st.sync()
            rcs.append(rc)
            algos.append(comm.info()["last_algo"])
            exp = np.concatenate(blocks) if coll == "ga" else blocks[rank]
            bad.append(int((seen.download(np.uint8, rb) != exp).sum()) if reads else 0)
        out = {"rcs": rcs, "bad": bad, "algos": algos}
        out.update(_info_fields(comm))
        for x in (send, recv, seen, word):
            x.free()
        st.destroy()
        out["destroy"] = comm.destroy()
        out_q.put((rank, out))
    except Exception:
        out_q.put((rank, {"error": traceback.format_exc()}))


def graph_rank(rank, n, port, env, cases, replays, out_q, barrier=None):
    """Each case (coll, algo, root, count, inplace) in turn on one communicator: ONE call captured into
    a HIP graph (the buffers hold a first seed's bytes, which no replay expects), replayed `replays`
    times with new bytes and every buffer refilled before each replay.  Then a call on pageable
    buffers under capture (refused: ncclInvalidUsage, nothing captured) and an eager call of each
    collective, checked: the counters are still in step."""
    try:
        hip_rt, M, comm = _open(rank, n, port, env)
        st = hip_rt.Stream()
        results = []
        for case in cases:
            comm.set_algo(case["algo"])
            call = GSCall(hip_rt, case["coll"], n, rank, case["count"], "f32", case["root"], case.get("inplace", False),
                          null=rank % 2 == 1)
            call.prepare(case["seed"])
            hip_rt.sync()
            _wait(barrier)
            rcs = []
            g = hip_rt.Graph(st, lambda: rcs.append(call.issue(comm, st)))
            res = {"case": case, "capture_rc": rcs, "captured_algo": comm.info()["last_algo"], "bad": [], "detail": []}
            for k in range(replays):
                call.prepare(case["seed"] + 1000 * (k + 1))
                hip_rt.sync()
                _wait(barrier)
                g.launch()
                st.sync()
                b, d = call.check()
                res["bad"].append(b)
                res["detail"].append(d)
            g.destroy()
            call.free()
            res.update(_info_fields(comm))
            results.append(res)
        # pageable buffers cannot be captured: every rank is refused before anything is negotiated
        comm.set_algo(M.ALGO_AUTO)
        refused = []
        for coll in ("ga", "sc"):
            call = GSCall(hip_rt, coll, n, rank, 4099, "f32", 0, mem="pageable")
            call.prepare(5)
            _wait(barrier)
            L, graph = hip_rt.lib(), ctypes.c_void_p()
            hip_rt.check(L.hipStreamBeginCapture(st.handle, 0), "hipStreamBeginCapture")
            try:
                refused.append(call.issue(comm, st))
            finally:
                hip_rt.check(L.hipStreamEndCapture(st.handle, ctypes.byref(graph)), "hipStreamEndCapture")
            if graph.value:
                L.hipGraphDestroy(graph)
            call.free()
        eager = []
        for i, coll in enumerate(("ga", "sc")):
            comm.set_algo((M.ALGO_RING, M.ALGO_READ)[i])
            res = _gs_case(hip_rt, comm, dict(coll=coll, count=4099, root=n - 1, seed=90 + i), rank, n, st, barrier, None)
            eager.append((res["rc"], res["bad"], res["algos"], res["detail"]))
        st.destroy()
        out_q.put((rank, {"results": results, "refused": refused, "eager": eager, "async": comm.async_error(),
                          "destroy": comm.destroy()}))
    except Exception:
        out_q.put((rank, {"error": traceback.format_exc()}))


def errors_rank(rank, n, port, env, scenario, out_q, barrier=None):
    """The calls the library must refuse, on device buffers under the read schedule (n = 2):
      root     -- the ranks disagree on the root (each names itself): ncclInvalidUsage on every rank;
      kinds    -- rank 0 calls Gather where rank 1 calls Scatter: ncclInvalidUsage;
      range    -- root = n, root = -1: ncclInvalidArgument;
      null     -- a buffer the rank's role needs is NULL: ncclInvalidArgument (every rank passes a
                  refusable call: the one-block buffer NULL everywhere, then the root lacking its large
                  buffer while the other rank lacks its one-block buffer);
      overlap  -- a partial overlap on the root (each rank names itself the root, so each is refused
                  before anything is negotiated): ncclInvalidArgument;
      dtype    -- ncclInt8: ncclInternalError;
      group    -- inside an open group: ncclInvalidUsage, and the group ends cleanly.
    Then the communicator's next valid calls succeed and are right."""
    try:
        hip_rt, M, comm = _open(rank, n, port, env)
        comm.set_algo(M.ALGO_READ)
        st = hip_rt.Stream()
        c = 4099
        b = c * 4
        small, big = hip_rt.DeviceBuffer(b), hip_rt.DeviceBuffer(n * b + 64)
        small.fill_byte(0)
        big.fill_byte(0)
        hip_rt.sync()
        _wait(barrier)
        F, h = M.ncclFloat, st.handle
        rcs, extra = [], {}
        if scenario == "root":
            rcs += [comm.gather(small.ptr, big.ptr, c, F, rank, h), comm.scatter(big.ptr, small.ptr, c, F, rank, h)]
        elif scenario == "kinds":
            rcs.append(comm.gather(small.ptr, big.ptr, c, F, 0, h) if rank == 0 else comm.scatter(big.ptr, small.ptr, c, F, 0, h))
        elif scenario == "range":
            rcs += [comm.gather(small.ptr, big.ptr, c, F, n, h), comm.gather(small.ptr, big.ptr, c, F, -1, h),
                    comm.scatter(big.ptr, small.ptr, c, F, n, h), comm.scatter(big.ptr, small.ptr, c, F, -1, h)]
        elif scenario == "null":
            root = 0
            rcs += [comm.gather(None, big.ptr, c, F, root, h), comm.scatter(big.ptr, None, c, F, root, h),
                    # the root lacks the side only it needs; the other rank lacks its own
                    comm.gather(small.ptr if rank == root else None, None, c, F, root, h),
                    comm.scatter(None, small.ptr if rank == root else None, c, F, root, h)]
        elif scenario == "overlap":
            rcs += [comm.gather(big.ptr + 8, big.ptr, c, F, rank, h), comm.scatter(big.ptr, big.ptr + 8, c, F, rank, h),
                    # the one-block buffer straddling two blocks of the large one
                    comm.gather(big.ptr + rank * b + 4, big.ptr, c, F, rank, h)]
        elif scenario == "dtype":
            rcs += [comm.gather(small.ptr, big.ptr, c, M.ncclInt8, 0, h), comm.scatter(big.ptr, small.ptr, c, M.ncclInt8, 0, h)]
        else:
            extra["group_start"] = M.group_start()
            rcs += [comm.gather(small.ptr, big.ptr, c, F, 0, h), comm.scatter(big.ptr, small.ptr, c, F, 0, h)]
            extra["group_end"] = M.group_end()
        out = {"rcs": rcs, "async_after": comm.async_error()}
        out.update(extra)
        # the communicator is still usable: a Gather to rank 1, then a Scatter from rank 0, checked
        nxt = [_gs_case(hip_rt, comm, dict(coll="ga", count=c, root=1, seed=70, null=True), rank, n, st, barrier, None),
               _gs_case(hip_rt, comm, dict(coll="sc", count=c, root=0, seed=71), rank, n, st, barrier, None)]
        out["next_rc"] = [x["rc"] for x in nxt]
        out["next_bad"] = [x["bad"] for x in nxt]
        out.update(_info_fields(comm))
        small.free()
        big.free()
        st.destroy()
        out["destroy"] = comm.destroy()
        out_q.put((rank, out))
    except Exception:
        out_q.put((rank, {"error": traceback.format_exc()}))


WINDOW_BYTES = 1 << 20


def windows_rank(rank, n, port, env, out_q, barrier=None):
    """MINI_NCCL_WINDOW_RENDEZVOUS=0, the read schedule.  Two registered windows; on one communicator a
    window all-reduce (window_calls moves: the windows are live), a gather and a scatter whose buffers
    lie in the windows (negotiated: window_calls unchanged, the read schedule, exact), and a last
    window all-reduce."""
    try:
        import oracle_api as O
        hip_rt, M, comm = _open(rank, n, port, env)
        comm.set_algo(M.ALGO_READ)
        st = hip_rt.Stream()
        swin, rwin = hip_rt.DeviceBuffer(WINDOW_BYTES, fresh=True), hip_rt.DeviceBuffer(WINDOW_BYTES, fresh=True)
        hs, hr = comm.register(swin.ptr, WINDOW_BYTES), comm.register(rwin.ptr, WINDOW_BYTES)
        steps = []

        def all_reduce(seed):
            count = 3 * 4099
            xs = O.random_inputs(n, count, "f32", seed=seed)
            swin.upload(xs[rank])
            hip_rt.sync()
            _wait(barrier)
            w0 = comm.info()["window_calls"]
            rc = comm.all_reduce(swin.ptr, rwin.ptr, count, M.ncclFloat, M.ncclSum, st.handle)
            st.sync()
            got, exp = rwin.download(np.float32, count), O.allreduce(xs, "f32", "sum")[rank]
            steps.append({"what": "ar@window", "rc": rc, "bad": int((got.view(np.uint32) != exp.view(np.uint32)).sum()),
                          "detail": "", "algo": comm.info()["last_algo"], "window_calls": comm.info()["window_calls"] - w0})

        def in_window(coll, seed, slot, **kw):
            # fixed places, the same on every rank: 4-byte aligned, not 16-byte aligned
            off = slot * (256 << 10) + 4
            call = GSCall(hip_rt, coll, n, rank, 4099, "f32", window=(swin, off, rwin, off + 256), **kw)
            call.prepare(seed)
            hip_rt.sync()
            _wait(barrier)
            w0 = comm.info()["window_calls"]
            rc = call.issue(comm, st)
            st.sync()
            bad, detail = call.check() if rc == 0 else (-1, "")
            steps.append({"what": coll + "@window", "rc": rc, "bad": bad, "detail": detail, "algo": comm.info()["last_algo"],
                          "window_calls": comm.info()["window_calls"] - w0})

        all_reduce(900)
        in_window("ga", 910, 0, root=1)
        in_window("sc", 911, 1, root=2)
        in_window("ga", 912, 2, root=0, inplace=True)
        in_window("sc", 913, 3, root=1, inplace=True)
        all_reduce(920)
        out = {"steps": steps, "windows": comm.info()["windows"]}
        out.update(_info_fields(comm))
        out["deregister"] = [comm.deregister(hs), comm.deregister(hr)]
        st.destroy()
        out["destroy"] = comm.destroy()
        swin.free()
        rwin.free()
        out_q.put((rank, out))
    except Exception:
        out_q.put((rank, {"error": traceback.format_exc()}))
