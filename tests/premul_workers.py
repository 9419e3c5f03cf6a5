"""Rank processes for the pre-multiplied-sum GPU tests (one process = one rank; placement, spawning
and comparison are tests/gpu_workers.py's).  Expected values: tests/premul_ref.py, computed
in-process from the same seeded inputs -- never from the library.
"""
import os
import traceback

import numpy as np

from gpu_workers import compare, use_rank_device

GUARD = 256  # bytes past every recv, filled before the call and checked after it


def _setup(rank, n, port, env):
    os.environ.update(env)
    os.environ["MINI_NCCL_PORT"] = str(port)
    import hip_rt
    import mini_nccl as M
    import oracle_api as O
    import premul_ref as P
    use_rank_device(rank)
    return hip_rt, M, O, P, M.Comm(n, rank, "127.0.0.1")


def _expected(P, case, xs, rank):
    coll, dt, s = case["coll"], case["dtype"], case["s"]
    if coll == "ar":
        return P.allreduce_expect(xs, s, dt, rank, case.get("inplace", False))
    if coll == "rs":
        return P.reduce_scatter_expect(xs, s, dt, rank)
    return P.reduce_expect(xs, s, dt)


def _call(M, comm, case, send_ptr, recv_ptr, code, op, stream):
    n, c = comm.count(), case["chunk"]
    if case["coll"] == "rs":
        return comm.reduce_scatter(send_ptr, recv_ptr, c, code, op, stream)
    if case["coll"] == "rd":
        return comm.reduce(send_ptr, recv_ptr, n * c, code, op, case.get("root", 0), stream)
    return comm.all_reduce(send_ptr, recv_ptr, n * c + case.get("tail", 0), code, op, stream)


def premul_rank(rank, n, port, cases, env, out_q, barrier=None):
    """Run `cases` on one communicator, every call checked bit for bit.  A case: coll ("ar" / "rs" /
    "rd"), dtype, s (the scalar; None: plain ncclSum, for the routing comparison), chunk (elements per
    chunk: an all-reduce runs over n * chunk + tail, a reduce over n * chunk), tail, inplace, algo,
    root, seed, mem (device / pinned).  The op is created for the call and destroyed right after it
    was issued."""
    try:
        hip_rt, M, O, P, comm = _setup(rank, n, port, env)
        stream = hip_rt.Stream()
        results = []
        for case in cases:
            coll, dt, s, c = case["coll"], case["dtype"], case["s"], case["chunk"]
            inplace, root = case.get("inplace", False), case.get("root", 0)
            comm.set_algo(case["algo"])
            code, npd = O.DTYPES[dt]
            esz = np.dtype(npd).itemsize
            ns = n * c + (case.get("tail", 0) if coll == "ar" else 0)
            nr = c if coll == "rs" else ns
            mine = rank * c * esz if coll == "rs" else 0
            mem = case.get("mem", "device")
            if inplace:
                whole = hip_rt.buffer(mem, ns * esz + GUARD)
                send, recv = hip_rt.View(whole, 0, ns * esz), hip_rt.View(whole, mine, nr * esz)
                guard = hip_rt.View(whole, ns * esz, GUARD)
            else:
                sbuf, rbuf = hip_rt.buffer(mem, ns * esz), hip_rt.buffer(mem, nr * esz + GUARD)
                send, recv = hip_rt.View(sbuf, 0, ns * esz), hip_rt.View(rbuf, 0, nr * esz)
                guard = hip_rt.View(rbuf, nr * esz, GUARD)
                rbuf.fill_byte(0xAB)
            xs = P.inputs(n, ns, dt, case["seed"])
            if s is None:
                exp = O.allreduce(xs, dt, "sum", inplace=inplace)[rank]
            else:
                exp = _expected(P, case, xs, rank)
            send.upload(xs[rank])
            guard.upload(np.full(GUARD, 0xAB, np.uint8))
            hip_rt.sync()
            if barrier is not None:
                barrier.wait(120)
            g0 = comm.info()["read_grid_calls"]
            op = M.ncclSum if s is None else comm.redop_premul_sum(P.scalar_arg(s, dt), code)
            rc = _call(M, comm, case, send.ptr, recv.ptr, code, op, stream.handle)
            drc = 0 if s is None else comm.redop_destroy(op)
            stream.sync()
            ci = comm.info()
            bad, first, detail = -1, -1, ""
            if rc == 0:
                bad, first = 0, -1
                if coll != "rd" or rank == root:
                    got = recv.download(npd, nr)
                    bad, first = compare(got, exp, dt, True)
                    if bad:
                        detail = f"got {got[first]!r} expected {exp[first]!r}"
                elif not inplace:  # a non-root's recv is never touched
                    bad = int((recv.download(np.uint8, nr * esz) != 0xAB).sum())
                bad += int((guard.download(np.uint8, GUARD) != 0xAB).sum())
            results.append({"case": case, "rc": rc, "destroy_rc": drc, "bad": bad, "first": first, "detail": detail,
                            "algo": ci["last_algo"], "grid": ci["read_grid_calls"] - g0, "async": comm.async_error()})
            if inplace:
                whole.free()
            else:
                sbuf.free()
                rbuf.free()
        stream.destroy()
        info = comm.info()
        out_q.put((rank, {"results": results, "destroy": comm.destroy(), "info": info}))
    except Exception:
        out_q.put((rank, {"error": traceback.format_exc()}))


def one_rank(cases, env, port, out_q):
    """nranks == 1: the scale kernel.  A case: dtype, s, count, inplace."""
    try:
        hip_rt, M, O, P, comm = _setup(0, 1, port, env)
        stream = hip_rt.Stream()
        results = []
        for case in cases:
            dt, s, count = case["dtype"], case["s"], case["count"]
            code, npd = O.DTYPES[dt]
            esz = np.dtype(npd).itemsize
            x = P.inputs(1, count, dt, case["seed"])[0]
            sbuf, rbuf = hip_rt.DeviceBuffer(count * esz + GUARD), hip_rt.DeviceBuffer(count * esz + GUARD)
            sbuf.fill_byte(0xAB)
            rbuf.fill_byte(0xAB)
            sbuf.upload(x)
            hip_rt.sync()
            out = sbuf if case["inplace"] else rbuf
            op = comm.redop_premul_sum(P.scalar_arg(s, dt), code)
            rcs = []
            for coll in ("ar", "rs", "rd"):
                if coll == "ar":
                    rcs.append(comm.all_reduce(sbuf.ptr, out.ptr, count, code, op, stream.handle))
                elif coll == "rs":
                    rcs.append(comm.reduce_scatter(sbuf.ptr, out.ptr, count, code, op, stream.handle))
                else:
                    rcs.append(comm.reduce(sbuf.ptr, out.ptr, count, code, op, 0, stream.handle))
                if case["inplace"]:
                    break  # (a second in-place call would scale the scaled values)
            stream.sync()
            comm.redop_destroy(op)
            got = out.download(npd, count)
            bad, first = compare(got, P.one_rank_expect(x, s, dt), dt, True)
            bad += int((out.download(np.uint8, GUARD, count * esz) != 0xAB).sum())
            if not case["inplace"]:  # the input is left as it was
                bad += compare(sbuf.download(npd, count), x, dt, False)[0]
            results.append({"case": case, "rcs": rcs, "bad": bad, "first": first, "algo": comm.info()["last_algo"]})
            sbuf.free()
            rbuf.free()
        stream.destroy()
        out_q.put((0, {"results": results, "destroy": comm.destroy()}))
    except Exception:
        out_q.put((0, {"error": traceback.format_exc()}))


def window_rank(rank, n, port, env, scenario, out_q, barrier=None):
    """Registered windows launched without a rendezvous (MINI_NCCL_WINDOW_RENDEZVOUS=0).
      parity   -- an all-reduce with the op inside the windows, out of place and in place: bit-exact and
                  counted in window_calls;
      mismatch -- rank 0's op carries 0.5, the others' 0.25: the kernels' signatures differ."""
    try:
        hip_rt, M, O, P, comm = _setup(rank, n, port, env)
        st = hip_rt.Stream()
        wbytes = 4 << 20
        sbuf, rbuf = hip_rt.DeviceBuffer(wbytes, fresh=True), hip_rt.DeviceBuffer(wbytes, fresh=True)
        comm.register(sbuf.ptr, wbytes)
        comm.register(rbuf.ptr, wbytes)
        res = {}
        if scenario == "parity":
            bad, rcs, wc, algos = [], [], [], []
            for i, (dt, s, count, so, ro) in enumerate([("f32", 0.3, 100003, 0, 4096), ("bf16", -2.5, 70001, 8192, None),
                                                        ("f32", 1.0 / n, 100003, 256, None)]):
                code, npd = O.DTYPES[dt]
                inplace = ro is None
                xs = P.inputs(n, count, dt, 7700 + i)
                exp = P.allreduce_expect(xs, s, dt, rank, inplace)
                sbuf.upload(xs[rank], so)
                hip_rt.sync()
                barrier.wait(120)
                w0 = comm.info()["window_calls"]
                op = comm.redop_premul_sum(P.scalar_arg(s, dt), code)
                rcs.append(comm.all_reduce(sbuf.ptr + so, sbuf.ptr + so if inplace else rbuf.ptr + ro, count, code, op,
                                           st.handle))
                comm.redop_destroy(op)
                st.sync()
                got = (sbuf if inplace else rbuf).download(npd, count, so if inplace else ro)
                bad.append(compare(got, exp, dt, True)[0])
                ci = comm.info()
                wc.append(ci["window_calls"] - w0)
                algos.append(ci["last_algo"])
            res.update(bad=bad, rcs=rcs, wc=wc, algos=algos)
        else:
            count = 100003
            barrier.wait(120)
            op = comm.redop_premul_sum(0.5 if rank == 0 else 0.25, M.ncclFloat)
            res.update(rc=comm.all_reduce(sbuf.ptr, rbuf.ptr, count, M.ncclFloat, op, st.handle))
        res["info"] = comm.info()
        st.destroy()
        res["destroy"] = comm.destroy()
        sbuf.free()
        rbuf.free()
        out_q.put((rank, res))
    except Exception:
        out_q.put((rank, {"error": traceback.format_exc()}))


def _checked_allreduce(hip_rt, M, O, P, comm, st, n, rank, send, recv, count, op, s, seed, barrier):
    """One f32 all-reduce with `op` (scalar s) on fresh inputs: (rc, mismatches or -1)."""
    xs = P.inputs(n, count, "f32", seed)
    send.upload(xs[rank])
    hip_rt.sync()
    if barrier is not None:
        barrier.wait(120)
    rc = comm.all_reduce(send.ptr, recv.ptr, count, M.ncclFloat, op, st.handle)
    st.sync()
    if rc != 0:
        return rc, -1
    return rc, compare(recv.download(np.float32, count), P.allreduce_expect(xs, s, "f32", rank), "f32", True)[0]


def mismatch_rank(rank, n, port, env, out_q, barrier=None):
    """The read schedule's rendezvous: rank 0's op carries 0.5, the others' 0.25 -- ncclInvalidUsage on
    every rank, nothing written -- then a correct call, then equal scalars behind handles created in a
    different order on every rank; the same for ncclReduce's rendezvous."""
    try:
        hip_rt, M, O, P, comm = _setup(rank, n, port, env)
        comm.set_algo(M.ALGO_READ)
        st = hip_rt.Stream()
        count = 40001
        send, recv = hip_rt.DeviceBuffer(count * 4), hip_rt.DeviceBuffer(count * 4)
        res = {}
        xs = P.inputs(n, count, "f32", 7800)
        send.upload(xs[rank])
        recv.fill_byte(0xAB)
        hip_rt.sync()
        barrier.wait(120)
        bad_op = comm.redop_premul_sum(0.5 if rank == 0 else 0.25, M.ncclFloat)
        res["rc"] = comm.all_reduce(send.ptr, recv.ptr, count, M.ncclFloat, bad_op, st.handle)
        st.sync()
        res["written"] = int((recv.download(np.uint8, count * 4) != 0xAB).sum())
        res["rc_reduce"] = comm.reduce(send.ptr, recv.ptr, count, M.ncclFloat, bad_op, 0, st.handle)
        st.sync()
        res["written_reduce"] = int((recv.download(np.uint8, count * 4) != 0xAB).sum())
        res["async_after"] = comm.async_error()
        comm.redop_destroy(bad_op)
        # a correct call afterwards
        good = comm.redop_premul_sum(0.25, M.ncclFloat)
        res["next"] = _checked_allreduce(hip_rt, M, O, P, comm, st, n, rank, send, recv, count, good, 0.25, 7801, barrier)
        comm.redop_destroy(good)
        # the same two scalars behind different handle numbers on every rank
        a, b = (0.3, -2.5) if rank % 2 == 0 else (-2.5, 0.3)
        h1, h2 = comm.redop_premul_sum(a, M.ncclFloat), comm.redop_premul_sum(b, M.ncclFloat)
        by_scalar = {a: h1, b: h2}
        res["handles"] = (by_scalar[0.3], by_scalar[-2.5])
        res["swapped"] = [_checked_allreduce(hip_rt, M, O, P, comm, st, n, rank, send, recv, count, by_scalar[s], s,
                                             7802 + i, barrier) for i, s in enumerate((0.3, -2.5))]
        res["info"] = comm.info()
        send.free()
        recv.free()
        st.destroy()
        res["destroy"] = comm.destroy()
        out_q.put((rank, res))
    except Exception:
        out_q.put((rank, {"error": traceback.format_exc()}))


def handles_rank(rank, n, port, env, out_q, barrier=None):
    """The handle table and its refusals, a valid call after each; MINI_NCCL_BLOCKING=0 in env: an op
    destroyed right after its call was issued."""
    try:
        hip_rt, M, O, P, comm = _setup(rank, n, port, env)
        comm.set_algo(M.ALGO_READ)
        st = hip_rt.Stream()
        count = 30011
        send, recv = hip_rt.DeviceBuffer(count * 4), hip_rt.DeviceBuffer(count * 4)
        res, usable = {}, []

        def still_usable(seed):
            op = comm.redop_premul_sum(0.3, M.ncclFloat)
            usable.append(_checked_allreduce(hip_rt, M, O, P, comm, st, n, rank, send, recv, count, op, 0.3, seed, barrier))
            comm.redop_destroy(op)

        ops = [comm.redop_premul_sum_rc(1.0 + i, M.ncclFloat) for i in range(17)]
        res["create_rcs"] = [rc for rc, _ in ops]
        res["handles"] = [h for rc, h in ops if rc == 0]
        res["destroy_mid"] = comm.redop_destroy(res["handles"][7])
        res["recreate"] = comm.redop_premul_sum_rc(0.75, M.ncclFloat)
        res["full_again"] = comm.redop_premul_sum_rc(0.5, M.ncclFloat)[0]
        # the re-created op works, with its own scalar
        res["recreated_call"] = _checked_allreduce(hip_rt, M, O, P, comm, st, n, rank, send, recv, count,
                                                   res["recreate"][1], 0.75, 7900, barrier)
        res["destroy_all"] = [comm.redop_destroy(h) for h in res["handles"][:7] + res["handles"][8:] + [res["recreate"][1]]]
        still_usable(7901)
        # refusals in a collective
        f32_op = comm.redop_premul_sum(0.3, M.ncclFloat)
        res["wrong_dtype"] = [comm.all_reduce(send.ptr, recv.ptr, count // 2, M.ncclDouble, f32_op, st.handle),
                              comm.reduce_scatter(send.ptr, recv.ptr, count // n, M.ncclBfloat16, f32_op, st.handle),
                              comm.reduce(send.ptr, recv.ptr, count, M.ncclInt32, f32_op, 0, st.handle)]
        still_usable(7902)
        unknown = f32_op + 1
        res["unknown"] = [comm.all_reduce(send.ptr, recv.ptr, count, M.ncclFloat, unknown, st.handle),
                          comm.all_reduce(send.ptr, recv.ptr, count, M.ncclFloat, M.MNCCL_FIRST_USER_OP + 16, st.handle),
                          comm.reduce(send.ptr, recv.ptr, count, M.ncclFloat, 1 << 20, 0, st.handle)]
        still_usable(7903)
        res["destroy_builtin"] = [comm.redop_destroy(M.ncclSum), comm.redop_destroy(M.ncclAvg), comm.redop_destroy(unknown),
                                  comm.redop_destroy(-1)]
        still_usable(7904)
        res["device_residence"] = comm.redop_premul_sum_rc(0.3, M.ncclFloat, M.ncclScalarDevice)[0]
        res["bad_dtype"] = comm.redop_premul_sum_rc(3, M.ncclInt8)[0]
        res["local_reduce"] = M.local_reduce(recv.ptr, send.ptr, send.ptr, 16, M.ncclFloat, f32_op, st.handle)
        res["avg"] = comm.all_reduce(send.ptr, recv.ptr, count, M.ncclFloat, M.ncclAvg, st.handle)
        # destroyed right after the call was issued (stream-ordered mode when BLOCKING=0)
        xs = P.inputs(n, count, "f32", 7905)
        send.upload(xs[rank])
        hip_rt.sync()
        barrier.wait(120)
        rc = comm.all_reduce(send.ptr, recv.ptr, count, M.ncclFloat, f32_op, st.handle)
        drc = comm.redop_destroy(f32_op)
        again = comm.redop_premul_sum(-2.5, M.ncclFloat)  # the slot is handed out again, another scalar
        st.sync()
        bad = compare(recv.download(np.float32, count), P.allreduce_expect(xs, 0.3, "f32", rank), "f32", True)[0]
        res["early_destroy"] = (rc, drc, bad, again == f32_op)
        comm.redop_destroy(again)
        still_usable(7906)
        res["usable"] = usable
        res["async"] = comm.async_error()
        res["blocking"] = comm.info()["blocking"]
        send.free()
        recv.free()
        st.destroy()
        res["destroy"] = comm.destroy()
        out_q.put((rank, res))
    except Exception:
        out_q.put((rank, {"error": traceback.format_exc()}))


def graph_rank(rank, n, port, env, replays, out_q):
    """Capture an all-reduce with the op on the read schedule, destroy the op, replay on fresh inputs."""
    try:
        hip_rt, M, O, P, comm = _setup(rank, n, port, env)
        comm.set_algo(M.ALGO_READ)
        st = hip_rt.Stream()
        count, s = (1 << 16) + 3, 0.3
        send, recv = hip_rt.DeviceBuffer(count * 4), hip_rt.DeviceBuffer(count * 4)
        op = comm.redop_premul_sum(s, M.ncclFloat)
        rcs = []
        g = hip_rt.Graph(st, lambda: rcs.append(comm.all_reduce(send.ptr, recv.ptr, count, M.ncclFloat, op, st.handle)))
        captured_algo = comm.info()["last_algo"]
        drc = comm.redop_destroy(op)
        other = comm.redop_premul_sum(-7.0, M.ncclFloat)  # the freed slot, another scalar: the graph keeps its own
        bad = []
        for k in range(replays):
            xs = P.inputs(n, count, "f32", 7950 + k)
            send.upload(xs[rank])
            hip_rt.sync()
            g.launch()
            st.sync()
            bad.append(compare(recv.download(np.float32, count), P.allreduce_expect(xs, s, "f32", rank), "f32", True)[0])
        g.destroy()
        out_q.put((rank, {"capture_rc": rcs, "destroy_rc": drc, "reused": other == op, "bad": bad,
                          "captured_algo": captured_algo, "async": comm.async_error()}))
        send.free()
        recv.free()
        st.destroy()
        comm.destroy()
    except Exception:
        out_q.put((rank, {"error": traceback.format_exc()}))
