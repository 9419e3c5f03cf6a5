"""Rank processes for the lifecycle GPU tests of ncclReduceScatter ("rs"), ncclAllGather ("ag"),
ncclBroadcast ("bc"), ncclReduce ("rd") and ncclAllToAll ("a2a"): graph capture and replay, ranks as
threads of one process, one rank, calls chained across streams, destroy with calls in flight,
registered windows, send and recv in one allocation (placement, spawning and comparison are
tests/gpu_workers.py's; the eager per-case runners tests/rooted_workers.py's and
tests/alltoall_workers.py's).

Inputs and expectations (call_inputs / call_expect, pair_inputs / pair_expect) are functions of a
seed, so a replay or a round with another seed expects other data in every chunk: a stale own chunk,
own block or root copy cannot pass.  A Call lays one collective out on buffers and checks, after
every run of it: recv exact (gpu_workers.compare: bit for bit, NaN payloads of + and * excepted),
the 256 guard bytes past recv unchanged, the send unchanged where the call only reads it, and a
sentinel-filled buffer in place of the side a rooted call's non-root does not use unchanged.
"""
import os
import threading
import traceback

import numpy as np

import alltoall_workers as AW
import coll_workers as CW
import rooted_workers as RW
from coll_workers import GUARD, _info_fields
from gpu_workers import compare, make_inputs, use_rank_device

FILL = 0xAB
FIVE = ("rs", "ag", "bc", "rd", "a2a")


# ---------------------------------------------------------------- expectations (CPU: test_lifecycle_cpu.py)
def elems(coll, n, count):
    """(elements in send, elements in recv) of one call with `count` as the API takes it."""
    return {"rs": (n * count, count), "ag": (count, n * count), "a2a": (n * count, n * count)}.get(coll, (count, count))


def call_inputs(coll, seed, n, count, dtype):
    """Every rank's send for one call: alltoall_workers.my_send's seeded bytes for the all-to-all,
    gpu_workers.make_inputs' seeded values (rank r seeded seed + r) for the others."""
    import oracle_api as O
    _, npd = O.DTYPES[dtype]
    if coll == "a2a":
        bb = count * np.dtype(npd).itemsize
        return [AW.my_send(seed, r, n, bb).view(npd) for r in range(n)]
    return make_inputs(n, elems(coll, n, count)[0], dtype, seed, False)


def call_expect(coll, xs, rank, dtype, op="sum", root=0):
    """What `rank`'s recv holds after the call on inputs xs; None where the call leaves it alone (a
    Reduce's non-root).  One rank: the copy."""
    import rooted_ref
    n = len(xs)
    if n == 1:
        return xs[0]
    if coll in ("rs", "ag", "ar"):
        return CW.expected(coll, xs, rank, dtype, op)
    if coll == "bc":
        return xs[root]
    if coll == "rd":
        return rooted_ref.reduce_expect(xs, dtype, op) if rank == root else None
    c = xs[0].size // n
    return np.concatenate([xs[q][rank * c:(rank + 1) * c] for q in range(n)])


def expectations_of(case, n, seed):
    """(every rank's send, every rank's expected recv) of one case, computed once for all ranks."""
    dtype, op, root = case.get("dtype", "f32"), case.get("op", "sum"), case.get("root", 0)
    xs = call_inputs(case["coll"], seed, n, case["count"], dtype)
    return xs, [call_expect(case["coll"], xs, r, dtype, op, root) for r in range(n)]


PAIRS = ("rs_ag", "rd_bc", "a2a_a2a")


def pair_inputs(pair, seed, n, count):
    """Every rank's n * count f32 elements (seeded bytes for the all-to-all pair) for two calls in a
    row, the second fed with what the first wrote."""
    return call_inputs("a2a" if pair == "a2a_a2a" else "ar", seed, n, count if pair == "a2a_a2a" else n * count, "f32")


def pair_expect(pair, xs, rank):
    """What the second call's recv holds: reduce-scatter then all-gather, and Reduce then Broadcast
    from one root over a count that is a multiple of n, give the all-reduce's bits on every rank;
    two all-to-alls return the original buffer."""
    import oracle_api as O
    if pair == "a2a_a2a":
        return xs[rank]
    assert xs[0].size % len(xs) == 0
    return O.allreduce(xs, "f32", "sum")[rank]


# ---------------------------------------------------------------- one call on its buffers
class Call:
    """One collective call of `rank` laid out on buffers.
    layout: "separate" (two allocations), "inplace" (rs / ag as NCCL defines it, bc / rd with
    recv == send on the root; a rooted call's non-roots stay out of place), "one" (send and recv at
    disjoint offsets, a multiple of 256 bytes and at least 256 bytes apart, of ONE hipMalloc),
    "window" (window = (send window buffer, offset, recv window buffer, offset)).
    null: a rooted call's non-root passes NULL for the side its role does not use; otherwise a
    FILL-filled buffer that must come back unchanged."""

    def __init__(self, coll, n, rank, count, dtype="f32", op="sum", root=0, layout="separate", null=False,
                 mem="device", window=None):
        import hip_rt
        import oracle_api as O
        self.coll, self.n, self.rank, self.count, self.dtype, self.op, self.root = coll, n, rank, count, dtype, op, root
        self.code, self.npd = O.DTYPES[dtype]
        self.opc = O.OPS[op]
        esz = np.dtype(self.npd).itemsize
        self.ns, self.nr = elems(coll, n, count)
        sb, rb = self.ns * esz, self.nr * esz
        is_root = rank == root
        self.uses_send = coll != "bc" or is_root
        self.uses_recv = coll != "rd" or is_root
        self.arith = coll in ("rs", "rd", "ar") and op in ("sum", "prod")
        self.inplace = layout == "inplace" and (coll in ("rs", "ag", "ar") or (coll in ("bc", "rd") and is_root))
        assert not (layout == "inplace" and coll == "a2a")
        self.owned, self.fills, self.spare = [], [], None
        self.send = self.recv = self.guard = None
        if self.inplace:
            big, mine = max(sb, rb), rank * count * esz
            whole = hip_rt.buffer(mem, big + GUARD)
            self.owned.append(whole)
            self.send = hip_rt.View(whole, mine if coll == "ag" else 0, sb)
            self.recv = hip_rt.View(whole, mine if coll == "rs" else 0, rb)
            self.guard = hip_rt.View(whole, big, GUARD)
            self.fills.append(hip_rt.View(whole, 0, big + GUARD))
            return
        need_s, need_r = self.uses_send or not null, self.uses_recv or not null
        if layout == "one":
            roff = (sb + 255) // 256 * 256 + 256
            whole = hip_rt.DeviceBuffer(roff + rb + GUARD, fresh=True)
            self.owned.append(whole)
            sreg, rreg = hip_rt.View(whole, 0, sb), hip_rt.View(whole, roff, rb + GUARD)
        elif layout == "window":
            swin, soff, rwin, roff = window
            assert soff + sb <= swin.nbytes and roff + rb + GUARD <= rwin.nbytes
            sreg, rreg = hip_rt.View(swin, soff, sb), hip_rt.View(rwin, roff, rb + GUARD)
        else:
            sreg = hip_rt.buffer(mem, sb) if need_s else None
            rreg = hip_rt.buffer(mem, rb + GUARD) if need_r else None
            self.owned += [b for b in (sreg, rreg) if b is not None]
            sreg = hip_rt.View(sreg, 0, sb) if need_s else None
            rreg = hip_rt.View(rreg, 0, rb + GUARD) if need_r else None
        if need_s:
            self.send = sreg
            if not self.uses_send:
                self.spare = sreg
        if need_r:
            self.recv = hip_rt.View(rreg.owner, rreg.offset, rb)
            if self.uses_recv:
                self.guard = hip_rt.View(rreg.owner, rreg.offset + rb, GUARD)
            else:
                self.spare = rreg
            self.fills.append(rreg)
        if self.spare is sreg and sreg is not None:
            self.fills.append(sreg)

    def prepare(self, seed, shared=None):
        """New seeded inputs in send; recv, its guard and the sentinel refilled with FILL.  shared:
        (inputs, expectations per rank) computed once for every rank (expectations_of)."""
        if shared is not None:
            self.mine, self.exp = shared[0][self.rank], shared[1][self.rank]
        else:
            xs = call_inputs(self.coll, seed, self.n, self.count, self.dtype)
            self.mine = xs[self.rank]
            self.exp = call_expect(self.coll, xs, self.rank, self.dtype, self.op, self.root) if self.uses_recv else None
        for f in self.fills:
            if hasattr(f.owner, "view"):  # host memory: no hipMemset
                f.owner.view()[f.offset:f.offset + f.nbytes] = FILL
            else:
                f.fill_byte(FILL)
        if self.uses_send:
            self.send.upload(self.mine)

    def issue(self, comm, stream):
        sp = self.send.ptr if self.send is not None else None
        rp = self.recv.ptr if self.recv is not None else None
        c, h = self.count, stream.handle
        if self.coll == "bc":
            return comm.broadcast(sp, rp, c, self.code, self.root, h)
        if self.coll == "rd":
            return comm.reduce(sp, rp, c, self.code, self.opc, self.root, h)
        if self.coll == "a2a":
            return comm.all_to_all(sp, rp, c, self.code, h)
        return CW.call(comm, self.coll, sp, rp, c, self.code, self.opc, h)

    def check(self):
        """(mismatches, detail): recv, guard, the send where it is only read, the sentinel."""
        bad, detail = 0, ""
        if self.uses_recv:
            got = self.recv.download(self.npd, self.nr)
            b, f = compare(got, self.exp, self.dtype, self.arith)
            if b:
                # the chunks (of `count` elements) the mismatching elements lie in
                ne = (got.view(np.uint8).reshape(got.size, -1) != self.exp.view(np.uint8).reshape(got.size, -1)).any(axis=1)
                chunks = sorted({int(i) // self.count for i in np.flatnonzero(ne)})
                detail = f"{b} elements differ, first {f}: got {got[f]!r} expected {self.exp[f]!r}; in chunks {chunks}"
            g = int((self.guard.download(np.uint8, GUARD) != FILL).sum())
            if g:
                detail += f" {g} guard bytes written"
            bad += b + g
        if self.uses_send and not self.inplace:
            s = compare(self.send.download(self.npd, self.ns), self.mine, self.dtype, False)[0]
            if s:
                detail += f" {s} elements of the send changed"
            bad += s
        if self.spare is not None:
            s = int((self.spare.download(np.uint8, self.spare.nbytes) != FILL).sum())
            if s:
                detail += f" {s} bytes of the unused buffer written"
            bad += s
        return bad, detail

    def free(self):
        for b in self.owned:
            b.free()
        self.owned = []


def _call_of(case, n, rank, window=None):
    null = rank in case["null_ranks"] if "null_ranks" in case else rank % 2 == 1
    return Call(case["coll"], n, rank, case["count"], case.get("dtype", "f32"), case.get("op", "sum"),
                case.get("root", 0), case.get("layout", "separate"), null, case.get("mem", "device"), window)


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


# ---------------------------------------------------------------- 1. graph capture and replay
def graph_rank(rank, n, port, env, cases, replays, out_q, barrier=None):
    """Each case in turn on one communicator: capture ONE call into a HIP graph (the buffers hold a
    first seed's data, which no replay expects), replay it `replays` times with new seeded inputs
    and recv refilled before every replay, then one eager call of the same collective and one eager
    all-reduce: the counters are still in step."""
    try:
        hip_rt, M, comm = _open(rank, n, port, env)
        st = hip_rt.Stream()
        results = []
        for case in cases:
            comm.set_algo(case["algo"])
            seed = case["seed"]
            call = _call_of(case, n, rank)
            call.prepare(seed)
            hip_rt.sync()
            _wait(barrier)
            rcs = []
            g = hip_rt.Graph(st, lambda: rcs.append(call.issue(comm, st)))
            res = {"case": case, "capture_rc": rcs, "captured_algo": comm.info()["last_algo"], "bad": [], "detail": []}
            for k in range(replays):
                call.prepare(seed + 1000 * (k + 1))
                hip_rt.sync()
                _wait(barrier)
                g.launch()
                st.sync()
                b, d = call.check()
                res["bad"].append(b)
                res["detail"].append(f"replay {k}: {d}" if b else "")
            call.prepare(seed + 1000 * (replays + 1))
            hip_rt.sync()
            _wait(barrier)
            res["eager_rc"] = call.issue(comm, st)
            st.sync()
            res["eager_algo"] = comm.info()["last_algo"]
            res["eager_bad"], res["eager_detail"] = call.check()
            ar = Call("ar", n, rank, 3 * 4099 + 1)
            ar.prepare(seed + 77)
            hip_rt.sync()
            _wait(barrier)
            res["ar_rc"] = ar.issue(comm, st)
            st.sync()
            res["ar_bad"], res["ar_detail"] = ar.check()
            res.update(_info_fields(comm))
            g.destroy()
            ar.free()
            call.free()
            results.append(res)
        st.destroy()
        info = comm.info()
        out_q.put((rank, {"results": results, "destroy": comm.destroy(), "info": info}))
    except Exception:
        out_q.put((rank, {"error": traceback.format_exc()}))


class _Pair:
    """Two calls in a row, the second fed with what the first wrote: src -> mid -> out, three
    allocations, a guard past each.  rd_bc's non-roots pass NULL for the sides they do not use."""

    def __init__(self, hip_rt, M, pair, n, rank, count, root):
        self.pair, self.n, self.rank, self.count, self.root, self.M = pair, n, rank, count, root, M
        self.nb = n * count * 4
        self.mb = count * 4 if pair == "rs_ag" else self.nb
        self.src, self.mid, self.out = (hip_rt.DeviceBuffer(b + GUARD) for b in (self.nb, self.mb, self.nb))

    def prepare(self, seed):
        xs = pair_inputs(self.pair, seed, self.n, self.count)
        self.mine, self.exp = xs[self.rank], pair_expect(self.pair, xs, self.rank)
        for b in (self.src, self.mid, self.out):
            b.fill_byte(FILL)
        self.src.upload(self.mine)

    def issue(self, comm, streams):
        """The two calls, on streams[0] and streams[1]; returns [(rc, last_algo)] * 2."""
        M, c, n, F, S = self.M, self.count, self.n, self.M.ncclFloat, self.M.ncclSum
        src, mid, out, h0, h1 = self.src.ptr, self.mid.ptr, self.out.ptr, streams[0].handle, streams[1].handle
        is_root = self.rank == self.root
        if self.pair == "rs_ag":
            first = lambda: comm.reduce_scatter(src, mid, c, F, S, h0)
            second = lambda: comm.all_gather(mid, out, c, F, h1)
        elif self.pair == "rd_bc":
            first = lambda: comm.reduce(src, mid if is_root else None, n * c, F, S, self.root, h0)
            second = lambda: comm.broadcast(mid if is_root else None, out, n * c, F, self.root, h1)
        else:
            first = lambda: comm.all_to_all(src, mid, c, F, h0)
            second = lambda: comm.all_to_all(mid, out, c, F, h1)
        done = []
        for f in (first, second):
            rc = f()
            done.append((rc, comm.info()["last_algo"]))
        return done

    def check(self):
        got = self.out.download(np.float32, self.nb // 4)
        bad, first = compare(got, self.exp, "f32", self.pair != "a2a_a2a")
        detail = f"{bad} elements differ, first {first}: got {got[first]!r} expected {self.exp[first]!r}" if bad else ""
        guards = sum(int((b.download(np.uint8, GUARD, nb) != FILL).sum())
                     for b, nb in ((self.src, self.nb), (self.mid, self.mb), (self.out, self.nb)))
        src = compare(self.src.download(np.float32, self.nb // 4), self.mine, "f32", False)[0]
        if self.pair == "rd_bc" and self.rank != self.root:  # never passed: nobody wrote it
            guards += int((self.mid.download(np.uint8, self.mb) != FILL).sum())
        if guards or src:
            detail += f" {guards} guard / unused bytes written, {src} elements of the source changed"
        return bad + guards + src, detail

    def free(self):
        for b in (self.src, self.mid, self.out):
            b.free()


def graph_pair_rank(rank, n, port, env, pair, algo, count, root, replays, out_q, barrier=None):
    """Two calls captured together into one graph (_Pair), replayed with new inputs every time."""
    try:
        hip_rt, M, comm = _open(rank, n, port, env)
        comm.set_algo(algo)
        st = hip_rt.Stream()
        p = _Pair(hip_rt, M, pair, n, rank, count, root)
        p.prepare(300)
        hip_rt.sync()
        _wait(barrier)
        cap = []
        g = hip_rt.Graph(st, lambda: cap.extend(p.issue(comm, (st, st))))
        out = {"capture": cap, "bad": [], "detail": []}
        for k in range(replays):
            p.prepare(301 + k)
            hip_rt.sync()
            _wait(barrier)
            g.launch()
            st.sync()
            b, d = p.check()
            out["bad"].append(b)
            out["detail"].append(f"replay {k}: {d}" if b else "")
        out.update(_info_fields(comm))
        g.destroy()
        p.free()
        st.destroy()
        out["info"] = comm.info()
        out["destroy"] = comm.destroy()
        out_q.put((rank, out))
    except Exception:
        out_q.put((rank, {"error": traceback.format_exc()}))


# ---------------------------------------------------------------- 2. ranks as threads
def threaded_colls_proc(n, port, env, cases, out_q):
    """gpu_workers.threaded_ranks_proc for the five: n ranks as threads of ONE process on one GPU
    (raw peer pointers in one address space, no dma-buf), each with its own non-blocking stream.
    Every allocation, upload, fill, download and free happens between barriers while no kernel runs
    (a device-wide synchronisation would otherwise wait for another thread's kernel, which waits for
    this thread's).  Reports {rank: results}."""
    try:
        os.environ.update(env)
        os.environ["MINI_NCCL_PORT"] = str(port)
        import hip_rt
        import mini_nccl as M
        bar = threading.Barrier(n)
        out = {}
        # inputs and expectations once per case, shared by the rank threads
        prepared = [expectations_of(case, n, 500 + i) for i, case in enumerate(cases)]

        def rank_main(r):
            try:
                hip_rt.set_device(0)
                comm = M.Comm(n, r, "127.0.0.1")
                st = hip_rt.Stream()
                res = []
                for i, case in enumerate(cases):
                    call = _call_of(case, n, r)
                    call.prepare(500 + i, prepared[i])
                    comm.set_algo(case["algo"])
                    bar.wait(120)  # every thread prepared: no memset / copy / free from here on
                    rc = call.issue(comm, st)
                    st.sync()
                    bar.wait(120)  # every thread's kernel done
                    bad, detail = call.check() if rc == 0 else (-1, "")
                    res.append({"case": case, "rc": rc, "bad": bad, "detail": detail, "async": comm.async_error(),
                                "last_algo": comm.info()["last_algo"]})
                    call.free()
                    bar.wait(120)  # frees done before anyone's next call
                info = comm.info()
                st.destroy()
                out[r] = {"results": res, "ranks_on_device": info["ranks_on_device"],
                          "ipc_open_failures": info["ipc_open_failures"], "read_map_failures": info["read_map_failures"],
                          "destroy": comm.destroy()}
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


# ---------------------------------------------------------------- 3. one rank
def one_rank_proc(port, env, cases, out_q):
    """A communicator of one rank: every call is the copy and launches no kernel (last_algo stays
    -1); then the all-to-all's refused overlaps and count == 0 for all five, which write nothing."""
    try:
        hip_rt, M, comm = _open(0, 1, port, env)
        st = hip_rt.Stream()
        results = []
        for i, case in enumerate(cases):
            call = _call_of(case, 1, 0)
            call.prepare(600 + i)
            hip_rt.sync()
            rc = call.issue(comm, st)
            st.sync()
            bad, detail = call.check() if rc == 0 else (-1, "")
            results.append({"case": case, "rc": rc, "bad": bad, "detail": detail, "last_algo": comm.info()["last_algo"]})
            call.free()
        c = 4099
        a, b = hip_rt.DeviceBuffer(c * 4 + 64), hip_rt.DeviceBuffer(c * 4 + GUARD)
        mine = call_inputs("a2a", 650, 1, c, "f32")[0]
        b.fill_byte(FILL)
        a.fill_byte(FILL)
        a.upload(mine)
        hip_rt.sync()
        F, S, h = M.ncclFloat, M.ncclSum, st.handle
        refused = [comm.all_to_all(a.ptr, a.ptr, c, F, h), comm.all_to_all(a.ptr, a.ptr + 8, c, F, h),
                   comm.all_to_all(a.ptr + 16, a.ptr, c, F, h)]
        zero = [comm.reduce_scatter(a.ptr, b.ptr, 0, F, S, h), comm.all_gather(a.ptr, b.ptr, 0, F, h),
                comm.broadcast(a.ptr, b.ptr, 0, F, 0, h), comm.reduce(a.ptr, b.ptr, 0, F, S, 0, h),
                comm.all_to_all(a.ptr, b.ptr, 0, F, h)]
        st.sync()
        want_a = np.concatenate([mine.view(np.uint8), np.full(64, FILL, np.uint8)])
        touched = int((a.download(np.uint8, c * 4 + 64) != want_a).sum()) + int((b.download(np.uint8, c * 4 + GUARD) != FILL).sum())
        out = {"results": results, "refused": refused, "zero": zero, "touched": touched}
        out.update(_info_fields(comm))
        a.free()
        b.free()
        st.destroy()
        out["destroy"] = comm.destroy()
        out_q.put((0, out))
    except Exception:
        out_q.put((0, {"error": traceback.format_exc()}))


# ---------------------------------------------------------------- 4. chains across two streams
CHAINS = (("rs_ag", 23333), ("rd_bc", 17500), ("a2a_a2a", 23333))  # n = 3: at most 70001 elements per buffer


def chains_rank(rank, n, port, env, algo, rounds, out_q, barrier=None):
    """MINI_NCCL_BLOCKING=0.  Per round the three chains of CHAINS (rd_bc to and from root 1), the
    first call of each on stream A and the second, which reads what the first wrote, on stream B;
    every round on buffers of its own, so nothing synchronises with the host between the first call
    and the last."""
    try:
        hip_rt, M, comm = _open(rank, n, port, env)
        comm.set_algo(algo)
        sts = (hip_rt.Stream(), hip_rt.Stream())
        pairs = []
        for k in range(rounds):
            for i, (pair, count) in enumerate(CHAINS):
                p = _Pair(hip_rt, M, pair, n, rank, count, 1)
                p.prepare(700 + 10 * k + i)
                pairs.append(p)
        hip_rt.sync()
        _wait(barrier)
        calls = []
        for p in pairs:
            calls += p.issue(comm, sts)
        for st in sts:
            st.sync()
        out = {"calls": calls, "bad": [], "detail": []}
        for p in pairs:
            b, d = p.check()
            out["bad"].append(b)
            out["detail"].append(d)
            p.free()
        out.update(_info_fields(comm))
        for st in sts:
            st.destroy()
        out["info"] = comm.info()
        out["destroy"] = comm.destroy()
        out_q.put((rank, out))
    except Exception:
        out_q.put((rank, {"error": traceback.format_exc()}))


# ---------------------------------------------------------------- 5. destroy with calls in flight
def destroy_inflight_rank(rank, n, port, env, count, out_q, barrier=None):
    """gpu_workers.destroy_inflight_rank for the five's kernels: a reduce-scatter, a Broadcast from
    root 2 and an all-to-all queued on one stream (MINI_NCCL_BLOCKING=0), ncclCommDestroy at once,
    then a device synchronisation and every result checked."""
    try:
        hip_rt, M, comm = _open(rank, n, port, env)
        st = hip_rt.Stream()
        calls = [Call("rs", n, rank, count), Call("bc", n, rank, count, root=2, null=rank == 1), Call("a2a", n, rank, count)]
        for i, c in enumerate(calls):
            c.prepare(800 + i)
        hip_rt.sync()
        _wait(barrier)
        rcs, algos = [], []
        for c in calls:
            rcs.append(c.issue(comm, st))
            algos.append(comm.info()["last_algo"])
        fields = _info_fields(comm)  # host-side counters and the status word: no wait for the kernels
        rc_destroy = comm.destroy()  # no synchronisation before it
        hip_rt.sync()
        checks = [c.check() for c in calls]
        for c in calls:
            c.free()
        st.destroy()
        out_q.put((rank, dict(fields, rcs=rcs, algos=algos, destroy=rc_destroy, bad=[b for b, _ in checks],
                              detail=[d for _, d in checks])))
    except Exception:
        out_q.put((rank, {"error": traceback.format_exc()}))


# ---------------------------------------------------------------- 6. registered windows
WINDOW_BYTES = 1 << 20
WINDOW_SLOT = 96 << 10  # per call; the largest region below is 3 * 4099 * 4 + 256 bytes


def windows_rank(rank, n, port, env, out_q, barrier=None):
    """MINI_NCCL_WINDOW_RENDEZVOUS=0, the read schedule.  Two registered windows; on one communicator
    a window all-reduce (a fast record on the board), each of the five on sub-ranges of the windows
    (negotiated: window_calls unchanged), a window all-reduce, the five on buffers outside any window
    (the eager runners of rooted_workers / alltoall_workers), a last window all-reduce."""
    try:
        hip_rt, M, comm = _open(rank, n, port, env)
        comm.set_algo(M.ALGO_READ)
        st = hip_rt.Stream()
        swin, rwin = hip_rt.DeviceBuffer(WINDOW_BYTES, fresh=True), hip_rt.DeviceBuffer(WINDOW_BYTES, fresh=True)
        hs, hr = comm.register(swin.ptr, WINDOW_BYTES), comm.register(rwin.ptr, WINDOW_BYTES)
        steps = []
        slot = [0]

        def in_window(coll, seed, **kw):
            # fixed offsets, the same on every rank: 4-byte aligned, not 16-byte aligned from slot 1 on
            off = slot[0] * WINDOW_SLOT + 4 * slot[0]
            slot[0] += 1
            call = Call(coll, n, rank, kw.pop("count", 4099), layout="window", window=(swin, off, rwin, off + 256),
                        null=rank % 2 == 1, **kw)
            call.prepare(seed)
            hip_rt.sync()
            _wait(barrier)
            w0 = comm.info()["window_calls"]
            rc = call.issue(comm, st)
            st.sync()
            bad, detail = call.check() if rc == 0 else (-1, "")
            ci = comm.info()
            steps.append({"what": coll + "@window", "rc": rc, "bad": bad, "detail": detail, "algo": ci["last_algo"],
                          "window_calls": ci["window_calls"] - w0, "async": comm.async_error()})

        def outside(case):
            w0 = comm.info()["window_calls"]
            run = AW._a2a_case if case["coll"] == "a2a" else RW._rooted_case if case["coll"] in ("bc", "rd") else RW._unrooted_case
            res = run(comm, case, rank, n, st, barrier, np.random.default_rng(rank))
            steps.append({"what": case["coll"] + "@outside", "rc": res["rc"], "bad": res["bad"], "detail": res["detail"],
                          "algo": res["algos"][-1] if res["algos"] else None,
                          "window_calls": comm.info()["window_calls"] - w0, "async": res["async"]})

        in_window("ar", 900, count=3 * 4099 + 2)
        for i, coll in enumerate(FIVE):
            in_window(coll, 910 + i, root=1, count=3 * 4099 + 2 if coll in ("bc", "rd") else 4099)
        in_window("ar", 920, count=3 * 4099 + 2)
        for i, coll in enumerate(FIVE):
            outside(dict(coll=coll, dtype="f32", op="sum", count=4099, inplace=False, algo=M.ALGO_READ, root=2,
                         null=rank == 0, seed=930 + i))
        in_window("ar", 940, count=3 * 4099 + 2)
        out = {"steps": steps, "windows": comm.info()["windows"]}
        out.update(_info_fields(comm))
        out["deregister"] = [comm.deregister(hs), comm.deregister(hr)]
        out["windows_after"] = comm.info()["windows"]
        st.destroy()
        out["info"] = comm.info()
        out["destroy"] = comm.destroy()
        swin.free()
        rwin.free()
        out_q.put((rank, out))
    except Exception:
        out_q.put((rank, {"error": traceback.format_exc()}))


# ---------------------------------------------------------------- 7. any list of Call cases, eagerly
def cases_rank(rank, n, port, env, cases, out_q, barrier=None):
    """Each case (coll, algo, count, dtype, op, root, layout, null_ranks, calls) on one communicator:
    `calls` eager calls on the same buffers, new seeded inputs before each, every call checked."""
    try:
        hip_rt, M, comm = _open(rank, n, port, env)
        st = hip_rt.Stream()
        results = []
        for i, case in enumerate(cases):
            comm.set_algo(case["algo"])
            call = _call_of(case, n, rank)
            res = {"case": case, "rcs": [], "bad": [], "detail": [], "algos": [], "rounds": []}
            for k in range(case.get("calls", 1)):
                call.prepare(1000 + 10 * i + k)
                hip_rt.sync()
                _wait(barrier)
                r0 = comm.info()["read_rounds"]
                rc = call.issue(comm, st)
                st.sync()
                b, d = call.check() if rc == 0 else (-1, "")
                res["rcs"].append(rc)
                res["bad"].append(b)
                res["detail"].append(d)
                res["algos"].append(comm.info()["last_algo"])
                res["rounds"].append(comm.info()["read_rounds"] - r0)
            res.update(_info_fields(comm))
            call.free()
            results.append(res)
        st.destroy()
        info = comm.info()
        out_q.put((rank, {"results": results, "destroy": comm.destroy(), "info": info}))
    except Exception:
        out_q.put((rank, {"error": traceback.format_exc()}))
