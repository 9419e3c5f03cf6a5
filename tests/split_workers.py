"""Rank processes for the ncclCommSplit GPU tests (one process = one rank; placement, spawning and
comparison are tests/gpu_workers.py's).

Expected values come from the existing oracle over the MEMBERS' inputs in new-rank order: every
parent rank draws its input from the same seed (gpu_workers.make_inputs over the parent's ranks), a
child of members [m0, m1, ...] -- parent ranks, in the order of their new ranks -- must produce what
the oracle produces for [x[m0], x[m1], ...].  Every device buffer is a Fenced: its payload sits
between two 256-byte sentinels, checked after every step.
"""
import os
import threading
import traceback

import numpy as np

from gpu_workers import compare, make_inputs, use_rank_device

GUARD, FILL = 256, 0xAB
COUNT = 4099  # f32 elements: a vector body plus an element tail


def members_of(colors, keys, rank):
    """Parent ranks of `rank`'s group in new-rank order ([] for a negative color): the rule restated."""
    if colors[rank] < 0:
        return []
    return [q for _, q in sorted((keys[q], q) for q in range(len(colors)) if colors[q] == colors[rank])]


class Fenced:
    """[GUARD sentinel bytes][payload][GUARD sentinel bytes] in one device allocation."""

    def __init__(self, hip_rt, nbytes):
        self.nb = nbytes
        self.buf = hip_rt.DeviceBuffer(nbytes + 2 * GUARD)
        self.ptr = self.buf.ptr + GUARD
        self.put(None)

    def put(self, arr):
        whole = np.full(self.nb + 2 * GUARD, FILL, np.uint8)
        if arr is not None:
            b = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
            whole[GUARD:GUARD + b.size] = b
        self.buf.upload(whole)

    def get(self, npd, count):
        return self.buf.download(npd, count, GUARD)

    def fences_bad(self):
        whole = self.buf.download(np.uint8, self.nb + 2 * GUARD)
        return int((whole[:GUARD] != FILL).sum() + (whole[GUARD + self.nb:] != FILL).sum())

    def free(self):
        self.buf.free()


class Ctx:
    def __init__(self, hip_rt, M, O, stream, barrier):
        self.hip_rt, self.M, self.O, self.stream, self.barrier = hip_rt, M, O, stream, barrier

    def ready(self):
        """Every rank's host-side preparation is done before any rank enters the next call."""
        self.hip_rt.sync()
        if self.barrier is not None:
            self.barrier.wait(120)


def allreduce_on(cx, comm, xs, me, algo, count=COUNT):
    """One out-of-place f32 Sum all-reduce on `comm` (None: this rank only keeps step with the
    barrier) over the inputs `xs` of its members, this rank being member `me`."""
    if comm is None:
        cx.ready()
        return None
    send, recv = Fenced(cx.hip_rt, count * 4), Fenced(cx.hip_rt, count * 4)
    send.put(xs[me])
    exp = cx.O.allreduce(xs, "f32", "sum")[me] if len(xs) > 1 else xs[0]  # one rank: a copy
    comm.set_algo(algo)
    cx.ready()
    rc = comm.all_reduce(send.ptr, recv.ptr, count, cx.M.ncclFloat, cx.M.ncclSum, cx.stream.handle)
    cx.stream.sync()
    bad = compare(recv.get(np.float32, count), exp, "f32", True)[0] if rc == 0 else -1
    unchanged = int((send.get(np.float32, count).view(np.uint32) != xs[me].view(np.uint32)).sum())
    res = {"what": "ar", "algo": algo, "rc": rc, "bad": bad + unchanged, "fences": send.fences_bad() + recv.fences_bad(),
           "last_algo": comm.info()["last_algo"], "async": comm.async_error()}
    send.free()
    recv.free()
    return res


def allgather_on(cx, comm, xs, me, algo, count=COUNT):
    if comm is None:
        cx.ready()
        return None
    n = len(xs)
    send, recv = Fenced(cx.hip_rt, count * 4), Fenced(cx.hip_rt, n * count * 4)
    send.put(xs[me])
    comm.set_algo(algo)
    cx.ready()
    rc = comm.all_gather(send.ptr, recv.ptr, count, cx.M.ncclFloat, cx.stream.handle)
    cx.stream.sync()
    bad = compare(recv.get(np.float32, n * count), np.concatenate(xs), "f32", False)[0] if rc == 0 else -1
    res = {"what": "ag", "algo": algo, "rc": rc, "bad": bad, "fences": send.fences_bad() + recv.fences_bad(),
           "last_algo": comm.info()["last_algo"], "async": comm.async_error()}
    send.free()
    recv.free()
    return res


def exchange_on(cx, comm, me, seed, count=COUNT):
    """A grouped send + recv with the other rank of a 2-rank communicator: seeded random bytes."""
    M, peer, nb = cx.M, 1 - me, count * 4
    msg = lambda src: np.frombuffer(np.random.default_rng([seed, src]).bytes(nb), np.uint8)
    send, recv = Fenced(cx.hip_rt, nb), Fenced(cx.hip_rt, nb)
    send.put(msg(me))
    cx.ready()
    rcs = [M.group_start(), comm.send(send.ptr, count, M.ncclFloat, peer, cx.stream.handle),
           comm.recv(recv.ptr, count, M.ncclFloat, peer, cx.stream.handle), M.group_end()]
    cx.stream.sync()
    bad = int((recv.get(np.uint8, nb) != msg(peer)).sum() + (send.get(np.uint8, nb) != msg(me)).sum())
    res = {"what": "p2p", "rc": max(rcs), "rcs": rcs, "bad": bad, "fences": send.fences_bad() + recv.fences_bad(),
           "last_algo": comm.info()["last_algo"], "async": comm.async_error()}
    send.free()
    recv.free()
    return res


def _parent_inputs(n, seed, count=COUNT):
    return make_inputs(n, count, "f32", seed, False)


def _pick(xs, members):
    return [xs[m] for m in members]


# ---------------------------------------------------------------------------------- the scenarios
def order_scenario(cx, comm, rank, n):
    """6 ranks, color = rank % 2, key = -rank: two children of 3 in reversed order."""
    colors, keys = [r % 2 for r in range(n)], [-r for r in range(n)]
    mem = members_of(colors, keys, rank)
    rc, child = comm.split_rc(colors[rank], keys[rank])
    out = {"split_rc": rc, "members": mem, "steps": []}
    if child is None:
        return out
    me = mem.index(rank)
    out["child_rank"], out["child_count"], out["want_rank"] = child.rank(), child.count(), me
    ci = child.info()
    out["child_info"] = {k: ci[k] for k in ("rank", "nranks", "device", "ranks_on_device", "algo", "windows")}
    seed = 100
    for algo in (0, 2):  # forced ring, then forced read
        out["steps"].append(allreduce_on(cx, child, _pick(_parent_inputs(n, seed), mem), me, algo))
        out["steps"].append(allgather_on(cx, child, _pick(_parent_inputs(n, seed + 1), mem), me, algo))
        seed += 2
    for k in range(3):  # parent, child, parent, child, ...: the counters are independent
        out["steps"].append(dict(allreduce_on(cx, comm, _parent_inputs(n, seed), rank, -1), parent=True))
        out["steps"].append(allreduce_on(cx, child, _pick(_parent_inputs(n, seed + 1), mem), me, (0, 2)[k % 2]))
        seed += 2
    out["child_destroy"] = child.destroy()
    return out


def nocolor_scenario(cx, comm, rank, n):
    """3 ranks, rank 2 NCCL_SPLIT_NOCOLOR; then every rank its own color."""
    M = cx.M
    colors, keys = [0, 0, M.NCCL_SPLIT_NOCOLOR], [0, 0, 0]
    mem = members_of(colors, keys, rank)
    rc, child = comm.split_rc(colors[rank], keys[rank])
    out = {"split_rc": rc, "got_child": child is not None, "members": mem, "steps": []}
    me = mem.index(rank) if mem else -1
    if child is not None:
        out["child_rank"], out["child_count"], out["want_rank"] = child.rank(), child.count(), me
    xs = _parent_inputs(n, 200)
    out["steps"].append(allreduce_on(cx, child, _pick(xs, mem), me, 2))
    out["steps"].append(allgather_on(cx, child, _pick(xs, mem), me, 0))
    out["child_destroy"] = child.destroy() if child is not None else 0
    # every rank its own color: one-rank children, the out-of-place all-reduce is a copy
    rc1, single = comm.split_rc(10 + rank, 5)
    out["single_rc"], out["got_single"] = rc1, single is not None
    if single is not None:
        out["single_rank"], out["single_count"] = single.rank(), single.count()
        out["steps"].append(allreduce_on(cx, single, [xs[rank]], 0, -1))
        out["single_destroy"] = single.destroy()
    out["steps"] = [s for s in out["steps"] if s is not None]
    # the parent after both splits
    out["steps"].append(dict(allreduce_on(cx, comm, _parent_inputs(n, 201), rank, -1), parent=True))
    return out


def whole_scenario(cx, comm, rank, n):
    """4 ranks into 2 x 2: point to point, ncclAllToAllv, a pre-multiplied sum, a window -- on the child."""
    import premul_ref as P
    M, hip_rt, st = cx.M, cx.hip_rt, cx.stream
    colors, keys = [r // 2 for r in range(n)], list(range(n))
    mem = members_of(colors, keys, rank)
    me = mem.index(rank)
    s = 0.3
    pop = comm.redop_premul_sum(P.scalar_arg(s, "f32"), M.ncclFloat)  # the parent's, made BEFORE the split
    child = comm.split(colors[rank], keys[rank])
    out = {"child_rank": child.rank(), "child_count": child.count(), "want_rank": me, "steps": []}
    # 0. the parent's handle is not the child's: an unknown handle, ncclInternalError, nothing launched
    xs = _pick(make_inputs(n, 2 * COUNT, "f32", 320, False), mem)
    send, recv = Fenced(hip_rt, 2 * COUNT * 4), Fenced(hip_rt, COUNT * 4)
    send.put(xs[me])
    cx.ready()
    out["parent_handle"] = pop
    out["parent_handle_rc"] = child.reduce_scatter(send.ptr, recv.ptr, COUNT, M.ncclFloat, pop, st.handle)
    st.sync()
    out["parent_handle_touched"] = int((recv.get(np.uint8, COUNT * 4) != FILL).sum()) + recv.fences_bad()
    out["parent_handle_async"] = child.async_error()
    out["parent_handle_on_parent_destroy"] = comm.redop_destroy(pop)
    send.free()
    recv.free()
    # 1. a grouped send + recv between new ranks 0 and 1 (the child stayed usable)
    out["steps"].append(exchange_on(cx, child, me, 300 + colors[rank]))
    # 2. ncclAllToAllv with unequal counts: rank a sends cnt(a, b) elements to rank b, blocks contiguous
    cnt = lambda a, b: (4099, 300, 1003, 70)[2 * a + b]
    sc, rcnt = [cnt(me, q) for q in range(2)], [cnt(q, me) for q in range(2)]
    sd, rd = [0, sc[0]], [0, rcnt[0]]
    sends = [np.random.default_rng([310 + colors[rank], a]).uniform(-1, 1, cnt(a, 0) + cnt(a, 1)).astype(np.float32)
             for a in range(2)]
    send, recv = Fenced(hip_rt, sum(sc) * 4), Fenced(hip_rt, sum(rcnt) * 4)
    send.put(sends[me])
    exp = np.concatenate([sends[q][(0 if me == 0 else cnt(q, 0)):][:cnt(q, me)] for q in range(2)])
    cx.ready()
    rc = child.all_to_all_v(send.ptr, sc, sd, recv.ptr, rcnt, rd, M.ncclFloat, st.handle)
    st.sync()
    out["steps"].append({"what": "a2av", "rc": rc, "bad": compare(recv.get(np.float32, sum(rcnt)), exp, "f32", False)[0],
                         "fences": send.fences_bad() + recv.fences_bad(), "async": child.async_error()})
    send.free()
    recv.free()
    # 3. ncclReduceScatter with a pre-multiplied sum created on the child
    op = child.redop_premul_sum(P.scalar_arg(s, "f32"), M.ncclFloat)
    send, recv = Fenced(hip_rt, 2 * COUNT * 4), Fenced(hip_rt, COUNT * 4)
    send.put(xs[me])
    cx.ready()
    rc = child.reduce_scatter(send.ptr, recv.ptr, COUNT, M.ncclFloat, op, st.handle)
    st.sync()
    exp = P.reduce_scatter_expect(xs, s, "f32", me)
    out["steps"].append({"what": "premul_rs", "rc": rc, "bad": compare(recv.get(np.float32, COUNT), exp, "f32", True)[0],
                         "fences": send.fences_bad() + recv.fences_bad(), "async": child.async_error()})
    out["child_op_destroy"] = child.redop_destroy(op)
    send.free()
    recv.free()
    # 4. the read schedule on the child
    out["steps"].append(allreduce_on(cx, child, _pick(_parent_inputs(n, 330), mem), me, 2))
    # 5. mncclCommRegister of a window on the child, then one all-reduce in it
    xs = _pick(_parent_inputs(n, 340), mem)
    win = Fenced(hip_rt, COUNT * 4)
    win.put(xs[me])
    cx.ready()
    wrc, h = child.register_rc(win.ptr, COUNT * 4)
    out["register_rc"] = wrc
    if wrc == 0:
        out["child_windows"], out["parent_windows"] = child.info()["windows"], comm.info()["windows"]
        w0 = child.info()["window_calls"]
        cx.ready()
        rc = child.all_reduce(win.ptr, win.ptr, COUNT, M.ncclFloat, M.ncclSum, st.handle)
        st.sync()
        exp = cx.O.allreduce(xs, "f32", "sum", inplace=True)[me]
        out["steps"].append({"what": "window_ar", "rc": rc, "bad": compare(win.get(np.float32, COUNT), exp, "f32", True)[0],
                             "fences": win.fences_bad(), "async": child.async_error(),
                             "window_calls": child.info()["window_calls"] - w0})
        child.deregister(h)
    win.free()
    out["child_destroy"] = child.destroy()
    return out


def nested_scenario(cx, comm, rank, n):
    """4 ranks: 2 x 2, each child split into singletons; the parent destroyed first."""
    colors, keys = [r % 2 for r in range(n)], [0] * n
    mem = members_of(colors, keys, rank)
    me = mem.index(rank)
    child = comm.split(colors[rank], keys[rank])
    rc, single = child.split_rc(child.rank(), 0)
    out = {"single_rc": rc, "got_single": single is not None, "steps": []}
    if single is not None:
        out["single_rank"], out["single_count"] = single.rank(), single.count()
    out["steps"].append(allreduce_on(cx, child, _pick(_parent_inputs(n, 400), mem), me, 2))
    cx.ready()
    out["parent_destroy"] = comm.destroy()  # collective over the parent's ranks; the children live on
    out["steps"].append(allreduce_on(cx, child, _pick(_parent_inputs(n, 401), mem), me, 0))
    out["steps"].append(allreduce_on(cx, child, _pick(_parent_inputs(n, 402), mem), me, 2))
    if single is not None:
        out["steps"].append(allreduce_on(cx, single, [_parent_inputs(n, 403)[rank]], 0, -1))
    out["child_destroy"] = child.destroy()
    out["single_destroy"] = single.destroy() if single is not None else -1
    return out


def refusals_scenario(cx, comm, rank, n):
    """2 ranks: a split inside an open group, a negative color on every rank; a valid split after each."""
    M = cx.M
    out = {"steps": []}

    def valid_split(seed):
        rc, child = comm.split_rc(0, -rank)  # both ranks, reversed
        res = {"rc": rc, "got": child is not None}
        if child is not None:
            mem = [1, 0]
            res.update(rank=child.rank(), want=mem.index(rank))
            res["ar"] = allreduce_on(cx, child, _pick(_parent_inputs(n, seed), mem), mem.index(rank), 2)
            res["destroy"] = child.destroy()
        return res

    # 1. inside an open group: ncclInvalidUsage; the group stays open and clean and then runs a
    #    send / recv pair on the parent
    peer, nb = 1 - rank, COUNT * 4
    msg = lambda src: np.frombuffer(np.random.default_rng([500, src]).bytes(nb), np.uint8)
    send, recv = Fenced(cx.hip_rt, nb), Fenced(cx.hip_rt, nb)
    send.put(msg(rank))
    cx.ready()
    rcs = [M.group_start()]
    rc, child = comm.split_rc(0, 0)
    out["in_group_rc"], out["in_group_child"] = rc, child is not None
    rcs += [comm.send(send.ptr, COUNT, M.ncclFloat, peer, cx.stream.handle),
            comm.recv(recv.ptr, COUNT, M.ncclFloat, peer, cx.stream.handle), M.group_end()]
    cx.stream.sync()
    out["group_rcs"] = rcs
    out["group_bad"] = int((recv.get(np.uint8, nb) != msg(peer)).sum()) + send.fences_bad() + recv.fences_bad()
    send.free()
    recv.free()
    out["after_group"] = valid_split(501)
    # 2. a negative color other than NCCL_SPLIT_NOCOLOR, on every rank (nobody enters the exchange)
    rc, child = comm.split_rc(-2, 0)
    out["negative_rc"], out["negative_child"] = rc, child is not None
    out["after_negative"] = valid_split(502)
    out["steps"].append(dict(allreduce_on(cx, comm, _parent_inputs(n, 503), rank, -1), parent=True))
    return out


def residency_scenario(cx, comm, rank, n):
    """8 ranks, MINI_NCCL_CHANNELS=512, 2 x 4: the residency cap is the family's.  The comparison comes
    first: a child whose run_pipelines exceeds its parent's launches NOTHING."""
    colors, keys = [r // 4 for r in range(n)], list(range(n))
    mem = members_of(colors, keys, rank)
    me = mem.index(rank)
    child = comm.split(colors[rank], keys[rank])
    pi, ci = comm.info(), child.info()
    keep = ("pipelines", "run_pipelines", "ranks_on_device", "nranks")
    out = {"parent": {k: pi[k] for k in keep}, "child": {k: ci[k] for k in keep}, "steps": [], "launched": False}
    # every rank sees every rank's verdict before anything is launched: the parent's records are the
    # same everywhere, so the comparison gives the same answer on every rank
    if ci["run_pipelines"] <= pi["run_pipelines"]:
        out["launched"] = True
        count = (1 << 20) + 3
        for k, algo in enumerate((0, 2)):
            xs = _pick(make_inputs(n, count, "f32", 600 + k, False), mem)
            out["steps"].append(allreduce_on(cx, child, xs, me, algo, count))
    out["child_destroy"] = child.destroy()
    return out


SCENARIOS = {"order": order_scenario, "nocolor": nocolor_scenario, "whole": whole_scenario, "nested": nested_scenario,
             "refusals": refusals_scenario, "residency": residency_scenario}


def split_rank(rank, n, port, env, scenario, out_q, barrier=None):
    """One parent communicator of n ranks, then SCENARIOS[scenario] on it."""
    try:
        os.environ.update(env)
        os.environ["MINI_NCCL_PORT"] = str(port)
        import hip_rt
        import mini_nccl as M
        import oracle_api as O
        use_rank_device(rank)
        comm = M.Comm(n, rank, "127.0.0.1")
        stream = hip_rt.Stream()
        out = SCENARIOS[scenario](Ctx(hip_rt, M, O, stream, barrier), comm, rank, n)
        stream.destroy()
        if comm.handle:
            out["parent_info"] = {k: v for k, v in comm.info().items() if k in ("device", "ranks_on_device", "windows")}
            out["parent_async"] = comm.async_error()
        out.setdefault("parent_destroy", comm.destroy())
        out_q.put((rank, out))
    except Exception:
        out_q.put((rank, {"error": traceback.format_exc()}))


def threaded_split_proc(n, port, env, out_q):
    """4 ranks as threads of ONE process on one GPU, split 2 x 2: both children's leaders live in one
    pid, so their read-schedule boards must not share a name.  One all-reduce on each child on the
    read schedule.  Every allocation, upload and download happens between barriers while no kernel
    runs (gpu_workers.threaded_ranks_proc's rule)."""
    try:
        os.environ.update(env)
        os.environ["MINI_NCCL_PORT"] = str(port)
        import hip_rt
        import mini_nccl as M
        import oracle_api as O
        bar = threading.Barrier(n)
        out = {}
        colors, keys = [r % 2 for r in range(n)], [-r for r in range(n)]
        xs_all = [_parent_inputs(n, 700 + k) for k in range(2)]

        def rank_main(r):
            try:
                hip_rt.set_device(0)
                comm = M.Comm(n, r, "127.0.0.1")
                st = hip_rt.Stream()
                mem = members_of(colors, keys, r)
                me = mem.index(r)
                rc, child = comm.split_rc(colors[r], keys[r])
                res = {"split_rc": rc, "got_child": child is not None, "steps": []}
                if child is None:
                    raise RuntimeError(f"ncclCommSplit returned {rc}")
                res.update(child_rank=child.rank(), child_count=child.count(), want_rank=me)
                child.set_algo(M.ALGO_READ)
                for k in range(2):
                    xs = _pick(xs_all[k], mem)
                    exp = O.allreduce(xs, "f32", "sum")[me]
                    send, recv = Fenced(hip_rt, COUNT * 4), Fenced(hip_rt, COUNT * 4)
                    send.put(xs[me])
                    hip_rt.sync()
                    bar.wait(120)  # every thread prepared: no copy / memset / free from here on
                    arc = child.all_reduce(send.ptr, recv.ptr, COUNT, M.ncclFloat, M.ncclSum, st.handle)
                    st.sync()
                    bar.wait(120)  # every thread's kernel done
                    res["steps"].append({"what": "ar", "algo": 2, "rc": arc,
                                         "bad": compare(recv.get(np.float32, COUNT), exp, "f32", True)[0],
                                         "fences": send.fences_bad() + recv.fences_bad(),
                                         "last_algo": child.info()["last_algo"], "async": child.async_error()})
                    send.free()
                    recv.free()
                    bar.wait(120)
                st.destroy()
                res["child_destroy"] = child.destroy()
                res["parent_destroy"] = comm.destroy()
                out[r] = res
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


def timing_rank(rank, n, ports, env, reps, out_q, barrier=None):
    """Wall time of one n-rank split into two halves against one ncclCommInitRank of n / 2 ranks (what
    a caller without ncclCommSplit does: a second port per group, ports[1:]), `reps` times each, in one run."""
    import time
    try:
        os.environ.update(env)
        os.environ["MINI_NCCL_PORT"] = str(ports[0])
        import hip_rt
        import mini_nccl as M
        use_rank_device(rank)
        comm = M.Comm(n, rank, "127.0.0.1")
        half, group = n // 2, rank // (n // 2)
        split_s, init_s = [], []
        for k in range(reps):
            barrier.wait(120)
            t0 = time.perf_counter()
            child = comm.split(group, rank)
            split_s.append(time.perf_counter() - t0)
            child.destroy()
            os.environ["MINI_NCCL_PORT"] = str(ports[1 + group])
            barrier.wait(120)
            t0 = time.perf_counter()
            second = M.Comm(half, rank % half, "127.0.0.1")
            init_s.append(time.perf_counter() - t0)
            second.destroy()
        out_q.put((rank, {"split_s": split_s, "init_s": init_s, "destroy": comm.destroy()}))
    except Exception:
        out_q.put((rank, {"error": traceback.format_exc()}))
